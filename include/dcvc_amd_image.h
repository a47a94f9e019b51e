/* dcvc_amd_image.h - picture files on the host: PNG pictures as packed 8-bit RGB (RGB24) or 16-bit RGB (rgb48), and YUV4MPEG2 (.y4m) headers (below).
 *
 * The reference reads and writes its RGB test sequences as PNG files through PIL (src/utils/video_reader.py:10-45
 * PNGReader: Image.open(path).convert('RGB'); src/utils/video_writer.py:9-30 PNGWriter: Image.fromarray(rgb).save(path)).
 * These entry points do the same on the host with zlib:
 *   reader: bit depth 8; colour types 0 (grey), 2 (RGB), 3 (palette), 4 (grey + alpha) and 6 (RGBA); all five row filters;
 *           any number of IDAT chunks; every chunk's CRC checked. Alpha is dropped and grey / palette pixels are expanded,
 *           as convert('RGB') does. 16-bit, sub-8-bit and interlaced files and truncated or corrupt ones are refused.
 *   writer: colour type 2, 8-bit, not interlaced, every row with filter 1 (Sub), zlib level DCVC_PNG_ZLIB_LEVEL. The pixels
 *           equal PIL's; the bytes of the file need not.
 * Returns 0, or -1 with dcvc_last_error() set (include/dcvc_amd_ops.h). */
#pragma once

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_PNG_ZLIB_LEVEL 1
#define DCVC_PNG_MAX_SIDE 16384

/* width and height of a PNG file (its header; the rest of the file is not read) */
int dcvc_png_info(const char* path, int* width, int* height);
/* decodes a PNG file into rgb (packed [height][width][3] u8, capacity bytes); width / height receive its size. A picture
 * larger than capacity is an error. */
int dcvc_png_read_rgb(const char* path, void* rgb, size_t capacity, int* width, int* height);
/* writes packed [height][width][3] u8 as a PNG file */
int dcvc_png_write_rgb(const char* path, const void* rgb, int width, int height);

/* 16-bit PNG <-> packed u16 RGB (rgb48: native-endian samples in memory; the file's are big-endian). No reference counterpart.
 *   reader: bit depth 16; colour types 0, 2, 4 and 6 (grey replicated, alpha dropped, as at 8 bits); all five row filters with
 *           the 16-bit filter unit (2, 4, 6 or 8 bytes per pixel); any number of IDAT chunks, every CRC checked. Interlaced
 *           and 8-bit files are refused. sBIT is ignored: a 16-bit PNG is always depth 16.
 *   writer: colour type 2, 16-bit, not interlaced, filter 1 (Sub) on every row, zlib level DCVC_PNG_ZLIB_LEVEL.
 * dcvc_png_info2 is dcvc_png_info for both kinds of file: bit_depth receives 8 or 16. */
int dcvc_png_info2(const char* path, int* width, int* height, int* bit_depth);
/* decodes a 16-bit PNG file into rgb16 (packed [height][width][3] u16, capacity bytes, 2-byte aligned) */
int dcvc_png_read_rgb16(const char* path, void* rgb16, size_t capacity, int* width, int* height);
/* writes packed [height][width][3] u16 as a 16-bit PNG file */
int dcvc_png_write_rgb16(const char* path, const void* rgb16, int width, int height);

/* YUV4MPEG2 (.y4m) headers, host only; the pictures behind them are raw planar samples (DCVC_PIX_* layouts of
 * include/dcvc_amd_ops.h, LSB-aligned u16 little-endian above 8 bits), each behind a "FRAME" line.
 *   accepted: "YUV4MPEG2", then the fields W H F I A C X in any order up to '\n' within 1024 bytes. C420jpeg | C420mpeg2 |
 *             C420paldv | C420 (also when C is absent), C422, C444 and C4xxpN for N in 9..16; Ip, I? or no I field. A and X
 *             are skipped; F absent or 0:0 reads as 25:1. Chroma siting (jpeg / mpeg2 / paldv) is ignored: chroma is
 *             up-sampled nearest-neighbour whatever the file says.
 *   refused, naming the offending field: interlaced It | Ib | Im; Cmono*, C411, C444alpha and unknown tags; unknown fields;
 *             non-positive or odd sides; a missing W or H.
 * pix_fmt is a DCVC_PIX_* value, header_bytes the length of the header line with its '\n'. */
typedef struct { int width, height, fps_num, fps_den, pix_fmt, bit_depth; long long header_bytes; } dcvc_y4m_info;
int dcvc_y4m_parse_header(const void* bytes, size_t n, dcvc_y4m_info* out);
/* as dcvc_y4m_parse_header, but field-interlaced material is accepted and reported (dcvc encode --deinterlace):
 * *interlacing = 0 for Ip, I? or no I field, 1 for It (top field first), 2 for Ib (bottom field first). Im (mixed) stays
 * refused. */
int dcvc_y4m_parse_header_i(const void* bytes, size_t n, dcvc_y4m_info* out, int* interlacing);
/* length of a "FRAME...\n" line (parameters included), < 0 if it is none */
int dcvc_y4m_frame_header_bytes(const void* bytes, size_t n);
/* writes "YUV4MPEG2 W.. H.. F..:.. Ip C..\n" (8-bit 4:2:0 as C420jpeg; header_bytes is not read); returns the bytes written.
 * DCVC_PIX_NV12 is refused: Y4M has no tag for it. */
int dcvc_y4m_write_header(char* dst, size_t cap, const dcvc_y4m_info* info);

#ifdef __cplusplus
}
#endif
