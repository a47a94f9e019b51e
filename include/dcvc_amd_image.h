/* dcvc_amd_image.h - PNG pictures as packed 8-bit RGB (RGB24) in host memory.
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

#ifdef __cplusplus
}
#endif
