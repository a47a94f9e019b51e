// png.cpp - PNG <-> packed RGB24, and 16-bit PNG <-> packed u16 RGB (rgb48), on the host (include/dcvc_amd_image.h), with zlib
// for the deflate stream.
//
// The reference's PNGReader / PNGWriter (src/utils/video_reader.py:10-45, video_writer.py:9-30) go through PIL:
// Image.open(path).convert('RGB') and Image.fromarray(rgb).save(path). The contract kept here is pixel equality with
// those: grey and palette pixels are expanded and alpha is dropped on reading; the writer stores 8-bit RGB.
// The file comes from the user: every length is checked against what is left before it is used, every CRC is checked,
// and the inflated data must cover every row the header implies.
#include "dcvc_amd_image.h"

#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_common.h"

namespace {

const uint8_t kSignature[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};

uint32_t be32(const uint8_t* p) { return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | p[3]; }

void put_be32(std::vector<uint8_t>& out, uint32_t v)
{
    const uint8_t b[4] = {uint8_t(v >> 24), uint8_t(v >> 16), uint8_t(v >> 8), uint8_t(v)};
    out.insert(out.end(), b, b + 4);
}

[[noreturn]] void fail(const std::string& path, const std::string& what) { throw std::runtime_error(path + ": " + what); }

std::vector<uint8_t> read_file(const std::string& path, size_t limit)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) fail(path, "cannot open");
    std::vector<uint8_t> data;
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, limit ? std::min(sizeof(buf), limit - data.size()) : sizeof(buf), f)) > 0) {
        data.insert(data.end(), buf, buf + n);
        if (limit && data.size() >= limit) break;
    }
    const bool err = ferror(f) != 0;
    fclose(f);
    if (err) fail(path, "read error");
    return data;
}

struct Header {
    int width = 0, height = 0, depth = 0, colour = 0, interlace = 0;
};

int channels_of(int colour)
{
    switch (colour) {
    case 0: return 1;
    case 2: return 3;
    case 3: return 1;
    case 4: return 2;
    case 6: return 4;
    default: return 0;
    }
}

// signature + IHDR (the first chunk, CRC checked); refuses what the reader does not decode. want_depth: 8 (the RGB24 entry
// points), 16 (the rgb48 ones) or 0 (either: dcvc_png_info2)
Header parse_header(const std::string& path, const std::vector<uint8_t>& d, int want_depth = 8)
{
    if (d.size() < 8 || std::memcmp(d.data(), kSignature, 8) != 0) fail(path, "not a PNG file");
    if (d.size() < 8 + 8 + 13 + 4) fail(path, "truncated (header)");
    const uint8_t* c = d.data() + 8;
    if (be32(c) != 13 || std::memcmp(c + 4, "IHDR", 4) != 0) fail(path, "the first chunk is not a valid IHDR");
    if (static_cast<uint32_t>(crc32(0L, c + 4, 17)) != be32(c + 21)) fail(path, "CRC mismatch in IHDR");
    const uint8_t* p = c + 8;
    const uint32_t w = be32(p), h = be32(p + 4);
    Header hd;
    hd.depth = p[8]; hd.colour = p[9]; hd.interlace = p[12];
    if (w == 0 || h == 0) fail(path, "empty picture");
    if (w > DCVC_PNG_MAX_SIDE || h > DCVC_PNG_MAX_SIDE) {
        fail(path, "picture size " + std::to_string(w) + "x" + std::to_string(h) + " above " + std::to_string(DCVC_PNG_MAX_SIDE));
    }
    hd.width = static_cast<int>(w); hd.height = static_cast<int>(h);
    if (channels_of(hd.colour) == 0) fail(path, "unknown colour type " + std::to_string(hd.colour));
    if (want_depth == 8 && hd.depth != 8) fail(path, "bit depth " + std::to_string(hd.depth) + " is not supported (8-bit PNG only)");
    if (want_depth == 16 && hd.depth != 16) fail(path, "bit depth " + std::to_string(hd.depth) + " is not supported (16-bit PNG only)");
    if (want_depth == 0 && hd.depth != 8 && hd.depth != 16) fail(path, "bit depth " + std::to_string(hd.depth) + " is not supported (8- or 16-bit PNG)");
    if (hd.depth == 16 && hd.colour == 3) fail(path, "a palette picture cannot have bit depth 16");
    if (p[10] != 0 || p[11] != 0) fail(path, "unknown compression or filter method");
    if (hd.interlace != 0) fail(path, "interlaced PNG is not supported");
    return hd;
}

uint8_t paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
    return static_cast<uint8_t>(pa <= pb && pa <= pc ? a : (pb <= pc ? b : c));
}

// depth 8: rgb is packed u8; depth 16: packed native u16 (the file's samples are big-endian)
void decode(const std::string& path, uint8_t* rgb, size_t capacity, int* width, int* height, int depth = 8)
{
    const std::vector<uint8_t> d = read_file(path, 0);
    const Header hd = parse_header(path, d, depth);
    const size_t W = static_cast<size_t>(hd.width), H = static_cast<size_t>(hd.height);
    const size_t bs = depth == 16 ? 2 : 1;          // bytes per sample
    if (W * H * 3 * bs > capacity) fail(path, "picture " + std::to_string(W) + "x" + std::to_string(H) + " does not fit the buffer");
    const int chans = channels_of(hd.colour);
    const int ch = chans * static_cast<int>(bs);    // the filter unit: bytes per pixel (2, 4, 6 or 8 at 16 bits)
    std::vector<uint8_t> idat, plte;
    bool ended = false;
    size_t pos = 8;
    while (!ended) {
        if (d.size() - pos < 12) fail(path, "truncated (chunk header)");
        const uint32_t len = be32(d.data() + pos);
        const uint8_t* type = d.data() + pos + 4;
        if (len > d.size() - pos - 12) fail(path, "truncated (chunk data)");
        const uint8_t* body = type + 4;
        if (static_cast<uint32_t>(crc32(0L, type, len + 4)) != be32(body + len)) {
            fail(path, "CRC mismatch in chunk " + std::string(reinterpret_cast<const char*>(type), 4));
        }
        if (pos == 8) {
            // IHDR, parsed above
        } else if (std::memcmp(type, "IDAT", 4) == 0) {
            idat.insert(idat.end(), body, body + len);
        } else if (std::memcmp(type, "PLTE", 4) == 0) {
            if (len == 0 || len % 3 != 0 || len > 768) fail(path, "bad PLTE chunk");
            plte.assign(body, body + len);
        } else if (std::memcmp(type, "IEND", 4) == 0) {
            ended = true;
        } else if (std::memcmp(type, "IHDR", 4) == 0 || !(type[0] & 0x20)) {
            fail(path, "unexpected critical chunk " + std::string(reinterpret_cast<const char*>(type), 4));
        }
        pos += 12 + static_cast<size_t>(len);
    }
    if (idat.empty()) fail(path, "no image data");
    if (hd.colour == 3 && plte.empty()) fail(path, "palette picture without PLTE");
    // inflate into the filtered rows: exactly H * (1 + W * ch) bytes, ch bytes per pixel
    const size_t stride = W * ch, raw_bytes = H * (1 + stride);
    std::vector<uint8_t> raw(raw_bytes);
    if (idat.size() > 0xffffffffu || raw_bytes > 0xffffffffu) fail(path, "image data too large");
    z_stream zs;
    std::memset(&zs, 0, sizeof(zs));
    if (inflateInit(&zs) != Z_OK) fail(path, "inflateInit failed");
    zs.next_in = idat.data(); zs.avail_in = static_cast<uInt>(idat.size());
    zs.next_out = raw.data(); zs.avail_out = static_cast<uInt>(raw_bytes);
    const int zr = inflate(&zs, Z_FINISH);
    const size_t got = raw_bytes - zs.avail_out;
    inflateEnd(&zs);
    // Z_STREAM_END: complete; Z_BUF_ERROR with a full buffer: data beyond the last row, ignored (as libpng does)
    if (zr != Z_STREAM_END && zr != Z_BUF_ERROR) fail(path, "corrupt image data (zlib error " + std::to_string(zr) + ")");
    if (got != raw_bytes) fail(path, "truncated image data");
    // unfilter in place
    std::vector<uint8_t> zero(stride, 0);
    const uint8_t* prev = zero.data();
    for (size_t y = 0; y < H; ++y) {
        uint8_t* row = raw.data() + y * (1 + stride);
        const int f = row[0];
        uint8_t* cur = row + 1;
        switch (f) {
        case 0: break;
        case 1: for (size_t i = ch; i < stride; ++i) cur[i] = uint8_t(cur[i] + cur[i - ch]); break;
        case 2: for (size_t i = 0; i < stride; ++i) cur[i] = uint8_t(cur[i] + prev[i]); break;
        case 3:
            for (size_t i = 0; i < stride; ++i) cur[i] = uint8_t(cur[i] + ((i >= size_t(ch) ? cur[i - ch] : 0) + prev[i]) / 2);
            break;
        case 4:
            for (size_t i = 0; i < stride; ++i) {
                const int a = i >= size_t(ch) ? cur[i - ch] : 0, c = i >= size_t(ch) ? prev[i - ch] : 0;
                cur[i] = uint8_t(cur[i] + paeth(a, prev[i], c));
            }
            break;
        default: fail(path, "unknown row filter " + std::to_string(f) + " in row " + std::to_string(y));
        }
        prev = cur;
        if (depth == 16) {
            // grey is replicated and alpha dropped, as at 8 bits; big-endian samples -> native u16
            uint16_t* o16 = reinterpret_cast<uint16_t*>(rgb) + y * W * 3;
            const bool grey = chans < 3;
            for (size_t x = 0; x < W; ++x) {
                const uint8_t* px = cur + x * static_cast<size_t>(ch);
                for (int q = 0; q < 3; ++q) {
                    const uint8_t* sp = px + (grey ? 0 : 2 * q);
                    o16[3 * x + static_cast<size_t>(q)] = static_cast<uint16_t>((sp[0] << 8) | sp[1]);
                }
            }
            continue;
        }
        uint8_t* o = rgb + y * W * 3;
        switch (hd.colour) {
        case 2: std::memcpy(o, cur, stride); break;
        case 6: for (size_t x = 0; x < W; ++x) { o[3 * x] = cur[4 * x]; o[3 * x + 1] = cur[4 * x + 1]; o[3 * x + 2] = cur[4 * x + 2]; } break;
        case 0: for (size_t x = 0; x < W; ++x) o[3 * x] = o[3 * x + 1] = o[3 * x + 2] = cur[x]; break;
        case 4: for (size_t x = 0; x < W; ++x) o[3 * x] = o[3 * x + 1] = o[3 * x + 2] = cur[2 * x]; break;
        case 3:
            for (size_t x = 0; x < W; ++x) {
                const size_t e = 3 * static_cast<size_t>(cur[x]);
                if (e + 3 > plte.size()) fail(path, "palette index out of range");
                std::memcpy(o + 3 * x, plte.data() + e, 3);
            }
            break;
        }
    }
    *width = hd.width;
    *height = hd.height;
}

void put_chunk(std::vector<uint8_t>& out, const char* type, const uint8_t* body, size_t len)
{
    put_be32(out, static_cast<uint32_t>(len));
    const size_t start = out.size();
    out.insert(out.end(), type, type + 4);
    out.insert(out.end(), body, body + len);
    put_be32(out, static_cast<uint32_t>(crc32(0L, out.data() + start, static_cast<uInt>(len + 4))));
}

void encode(const std::string& path, const uint8_t* rgb, int width, int height)
{
    if (width <= 0 || height <= 0 || width > DCVC_PNG_MAX_SIDE || height > DCVC_PNG_MAX_SIDE) {
        fail(path, "picture size " + std::to_string(width) + "x" + std::to_string(height) + " out of range");
    }
    if (rgb == nullptr) fail(path, "no pixels");
    const size_t W = static_cast<size_t>(width), H = static_cast<size_t>(height), stride = 3 * W;
    std::vector<uint8_t> raw(H * (1 + stride));
    for (size_t y = 0; y < H; ++y) {              // filter 1 (Sub) on every row
        const uint8_t* s = rgb + y * stride;
        uint8_t* o = raw.data() + y * (1 + stride);
        o[0] = 1;
        for (size_t i = 0; i < 3 && i < stride; ++i) o[1 + i] = s[i];
        for (size_t i = 3; i < stride; ++i) o[1 + i] = uint8_t(s[i] - s[i - 3]);
    }
    uLongf zlen = compressBound(static_cast<uLong>(raw.size()));
    std::vector<uint8_t> z(zlen);
    if (compress2(z.data(), &zlen, raw.data(), static_cast<uLong>(raw.size()), DCVC_PNG_ZLIB_LEVEL) != Z_OK) fail(path, "deflate failed");
    std::vector<uint8_t> out(kSignature, kSignature + 8);
    uint8_t ihdr[13] = {};
    for (int k = 0; k < 4; ++k) { ihdr[k] = uint8_t(W >> (24 - 8 * k)); ihdr[4 + k] = uint8_t(H >> (24 - 8 * k)); }
    ihdr[8] = 8; ihdr[9] = 2;
    out.reserve(zlen + 64);
    put_chunk(out, "IHDR", ihdr, 13);
    put_chunk(out, "IDAT", z.data(), zlen);
    put_chunk(out, "IEND", nullptr, 0);
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) fail(path, "cannot write");
    const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    if (fclose(f) != 0 || !ok) fail(path, "write error");
}

// colour type 2, 16 bits: big-endian samples, filter 1 (Sub) on every row with the 6-byte pixel as its unit
void encode16(const std::string& path, const uint16_t* rgb, int width, int height)
{
    if (width <= 0 || height <= 0 || width > DCVC_PNG_MAX_SIDE || height > DCVC_PNG_MAX_SIDE) {
        fail(path, "picture size " + std::to_string(width) + "x" + std::to_string(height) + " out of range");
    }
    if (rgb == nullptr) fail(path, "no pixels");
    const size_t W = static_cast<size_t>(width), H = static_cast<size_t>(height), stride = 6 * W;
    std::vector<uint8_t> raw(H * (1 + stride)), line(stride);
    for (size_t y = 0; y < H; ++y) {
        const uint16_t* s = rgb + y * 3 * W;
        for (size_t i = 0; i < 3 * W; ++i) { line[2 * i] = uint8_t(s[i] >> 8); line[2 * i + 1] = uint8_t(s[i]); }
        uint8_t* o = raw.data() + y * (1 + stride);
        o[0] = 1;
        for (size_t i = 0; i < 6; ++i) o[1 + i] = line[i];
        for (size_t i = 6; i < stride; ++i) o[1 + i] = uint8_t(line[i] - line[i - 6]);
    }
    if (raw.size() > 0xffffffffu) fail(path, "image data too large");
    uLongf zlen = compressBound(static_cast<uLong>(raw.size()));
    std::vector<uint8_t> z(zlen);
    if (compress2(z.data(), &zlen, raw.data(), static_cast<uLong>(raw.size()), DCVC_PNG_ZLIB_LEVEL) != Z_OK) fail(path, "deflate failed");
    std::vector<uint8_t> out(kSignature, kSignature + 8);
    uint8_t ihdr[13] = {};
    for (int k = 0; k < 4; ++k) { ihdr[k] = uint8_t(W >> (24 - 8 * k)); ihdr[4 + k] = uint8_t(H >> (24 - 8 * k)); }
    ihdr[8] = 16; ihdr[9] = 2;
    out.reserve(zlen + 64);
    put_chunk(out, "IHDR", ihdr, 13);
    put_chunk(out, "IDAT", z.data(), zlen);
    put_chunk(out, "IEND", nullptr, 0);
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) fail(path, "cannot write");
    const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    if (fclose(f) != 0 || !ok) fail(path, "write error");
}

}  // namespace

extern "C" {

int dcvc_png_info(const char* path, int* width, int* height)
{
    return dcvc::guarded([&] {
        if (path == nullptr || width == nullptr || height == nullptr) throw std::invalid_argument("png_info: null argument");
        const Header hd = parse_header(path, read_file(path, 8 + 8 + 13 + 4));
        *width = hd.width;
        *height = hd.height;
    });
}

int dcvc_png_read_rgb(const char* path, void* rgb, size_t capacity, int* width, int* height)
{
    return dcvc::guarded([&] {
        if (path == nullptr || rgb == nullptr || width == nullptr || height == nullptr) throw std::invalid_argument("png_read_rgb: null argument");
        decode(path, static_cast<uint8_t*>(rgb), capacity, width, height);
    });
}

int dcvc_png_write_rgb(const char* path, const void* rgb, int width, int height)
{
    return dcvc::guarded([&] {
        if (path == nullptr) throw std::invalid_argument("png_write_rgb: null path");
        encode(path, static_cast<const uint8_t*>(rgb), width, height);
    });
}

int dcvc_png_info2(const char* path, int* width, int* height, int* bit_depth)
{
    return dcvc::guarded([&] {
        if (path == nullptr || width == nullptr || height == nullptr || bit_depth == nullptr) throw std::invalid_argument("png_info2: null argument");
        const Header hd = parse_header(path, read_file(path, 8 + 8 + 13 + 4), 0);
        *width = hd.width;
        *height = hd.height;
        *bit_depth = hd.depth;
    });
}

int dcvc_png_read_rgb16(const char* path, void* rgb16, size_t capacity, int* width, int* height)
{
    return dcvc::guarded([&] {
        if (path == nullptr || rgb16 == nullptr || width == nullptr || height == nullptr) throw std::invalid_argument("png_read_rgb16: null argument");
        if (reinterpret_cast<uintptr_t>(rgb16) & 1) throw std::invalid_argument("png_read_rgb16: the pixel buffer must be 2-byte aligned");
        decode(path, static_cast<uint8_t*>(rgb16), capacity, width, height, 16);
    });
}

int dcvc_png_write_rgb16(const char* path, const void* rgb16, int width, int height)
{
    return dcvc::guarded([&] {
        if (path == nullptr) throw std::invalid_argument("png_write_rgb16: null path");
        if (reinterpret_cast<uintptr_t>(rgb16) & 1) throw std::invalid_argument("png_write_rgb16: the pixel buffer must be 2-byte aligned");
        encode16(path, static_cast<const uint16_t*>(rgb16), width, height);
    });
}

}  // extern "C"
