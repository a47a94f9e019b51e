// y4m.cpp - YUV4MPEG2 (.y4m) stream and frame headers (include/dcvc_amd_image.h). Host only: the pictures behind the headers
// are raw planar samples, which the tool reads and writes itself.
//
// "YUV4MPEG2" then space-separated tagged fields up to '\n': W<width> H<height> F<num>:<den> I<interlacing> A<aspect>
// C<chroma> X<comment>; every picture is "FRAME" [parameters] '\n' followed by the planes Y, Cb, Cr.
#include "dcvc_amd_image.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "capi_common.h"
#include "dcvc_amd_ops.h"

namespace {

constexpr size_t kMaxHeader = 1024;
const char kMagic[] = "YUV4MPEG2";

[[noreturn]] void fail(const char* who, const std::string& msg) { throw std::invalid_argument(std::string(who) + ": " + msg); }

// a decimal number that fills s completely, 1 .. 2^30; -1 otherwise
long number(const std::string& s)
{
    if (s.empty() || s.size() > 10 || s.find_first_not_of("0123456789") != std::string::npos) return -1;
    const long long v = atoll(s.c_str());
    return v > (1 << 30) ? -1 : static_cast<long>(v);
}

void chroma_tag(const char* who, const std::string& tag, int& fmt, int& depth)
{
    const std::string field = "C" + tag;
    std::string base = tag;
    depth = 8;
    const size_t p = tag.find('p');
    // 4xxpN, N in 9..16 (420paldv is a siting name, not a depth)
    if (p == 3 && tag != "420paldv") {
        const long d = number(tag.substr(4));
        if (d < 9 || d > 16) fail(who, "unsupported chroma tag " + field + " (bit depths 9..16)");
        depth = static_cast<int>(d);
        base = tag.substr(0, 3);
    }
    if (base == "420" || (depth == 8 && (base == "420jpeg" || base == "420mpeg2" || base == "420paldv"))) fmt = DCVC_PIX_YUV420P;
    else if (base == "422") fmt = DCVC_PIX_YUV422P;
    else if (base == "444") fmt = DCVC_PIX_YUV444P;
    else fail(who, "unsupported chroma tag " + field + " (C420jpeg, C420mpeg2, C420paldv, C420, C422, C444 and their pN forms)");
}

// interlacing == nullptr: the entry that refuses interlaced material; else It -> 1, Ib -> 2 (Ip, I?, no I field: 0)
void parse_header(const void* bytes, size_t n, dcvc_y4m_info* out, int* interlacing)
{
    const char* who = "y4m_parse_header";
    if (bytes == nullptr || out == nullptr) fail(who, "null argument");
    int fields = 0;
    const char* p = static_cast<const char*>(bytes);
    const size_t ml = sizeof(kMagic) - 1;
    if (n < ml + 1 || std::memcmp(p, kMagic, ml) != 0 || (p[ml] != ' ' && p[ml] != '\n')) fail(who, "no YUV4MPEG2 magic");
    const size_t lim = n < kMaxHeader ? n : kMaxHeader;
    const void* nl = std::memchr(p, '\n', lim);
    if (nl == nullptr) fail(who, "no end of the header line within " + std::to_string(lim) + " bytes");
    const size_t len = static_cast<size_t>(static_cast<const char*>(nl) - p);
    dcvc_y4m_info info;
    info.width = info.height = 0;
    info.fps_num = 25; info.fps_den = 1;
    info.pix_fmt = DCVC_PIX_YUV420P;
    info.bit_depth = 8;
    info.header_bytes = static_cast<long long>(len) + 1;
    bool has_w = false, has_h = false;
    size_t i = ml;
    while (i < len) {
        if (p[i] == ' ') { ++i; continue; }
        size_t e = i;
        while (e < len && p[e] != ' ') ++e;
        const std::string field(p + i, e - i), val = field.substr(1);
        i = e;
        switch (field[0]) {
        case 'W':
        case 'H': {
            const long v = number(val);
            if (v <= 0 || (v & 1)) fail(who, "field " + field + ": picture sides must be positive and even");
            (field[0] == 'W' ? info.width : info.height) = static_cast<int>(v);
            (field[0] == 'W' ? has_w : has_h) = true;
            break;
        }
        case 'F': {
            const size_t c = val.find(':');
            const long a = c == std::string::npos ? -1 : number(val.substr(0, c)), b = c == std::string::npos ? -1 : number(val.substr(c + 1));
            if (a < 0 || b < 0) fail(who, "field " + field + ": a rate num:den expected");
            if (a > 0 && b > 0) { info.fps_num = static_cast<int>(a); info.fps_den = static_cast<int>(b); }      // 0:0 = unknown
            break;
        }
        case 'I':
            if (val == "p" || val == "?") fields = 0;
            else if (interlacing != nullptr && (val == "t" || val == "b")) fields = val == "t" ? 1 : 2;
            else fail(who, "field " + field + ": interlaced material is not supported");
            break;
        case 'C':
            chroma_tag(who, val, info.pix_fmt, info.bit_depth);
            break;
        case 'A':
        case 'X':
            break;
        default:
            fail(who, "unknown field " + field);
        }
    }
    if (!has_w) fail(who, "no W field");
    if (!has_h) fail(who, "no H field");
    *out = info;
    if (interlacing != nullptr) *interlacing = fields;
}

int write_header(char* dst, size_t cap, const dcvc_y4m_info* info)
{
    const char* who = "y4m_write_header";
    if (dst == nullptr || info == nullptr) fail(who, "null argument");
    if (info->width <= 0 || info->height <= 0 || (info->width & 1) || (info->height & 1)) fail(who, "picture sides must be positive and even");
    if (info->fps_num <= 0 || info->fps_den <= 0) fail(who, "the rate must be positive");
    if (info->bit_depth < 8 || info->bit_depth > 16) fail(who, "bit depth must be 8..16");
    const char* base = info->pix_fmt == DCVC_PIX_YUV420P ? "420" : info->pix_fmt == DCVC_PIX_YUV422P ? "422" :
                       info->pix_fmt == DCVC_PIX_YUV444P ? "444" : nullptr;
    if (base == nullptr) fail(who, "Y4M has no tag for pixel format " + std::to_string(info->pix_fmt) + " (planar formats only)");
    std::string tag = base;
    if (info->bit_depth > 8) tag += "p" + std::to_string(info->bit_depth);
    else if (info->pix_fmt == DCVC_PIX_YUV420P) tag += "jpeg";      // the tag most readers expect; the siting is not tracked
    char buf[160];
    const int len = snprintf(buf, sizeof(buf), "%s W%d H%d F%d:%d Ip C%s\n", kMagic, info->width, info->height, info->fps_num,
                             info->fps_den, tag.c_str());
    if (len < 0 || static_cast<size_t>(len) >= sizeof(buf) || static_cast<size_t>(len) > cap) fail(who, "the buffer is too small");
    std::memcpy(dst, buf, static_cast<size_t>(len));
    return len;
}

}  // namespace

extern "C" {

int dcvc_y4m_parse_header(const void* bytes, size_t n, dcvc_y4m_info* out)
{
    return dcvc::guarded([&] { parse_header(bytes, n, out, nullptr); });
}

int dcvc_y4m_parse_header_i(const void* bytes, size_t n, dcvc_y4m_info* out, int* interlacing)
{
    return dcvc::guarded([&] {
        if (interlacing == nullptr) fail("y4m_parse_header", "null argument");
        parse_header(bytes, n, out, interlacing);
    });
}

int dcvc_y4m_frame_header_bytes(const void* bytes, size_t n)
{
    int len = -1;
    const int rc = dcvc::guarded([&] {
        const char* who = "y4m_frame_header_bytes";
        if (bytes == nullptr) fail(who, "null argument");
        const char* p = static_cast<const char*>(bytes);
        if (n < 6 || std::memcmp(p, "FRAME", 5) != 0 || (p[5] != '\n' && p[5] != ' ')) fail(who, "no FRAME line");
        const size_t lim = n < kMaxHeader ? n : kMaxHeader;
        const void* nl = std::memchr(p, '\n', lim);
        if (nl == nullptr) fail(who, "no end of the FRAME line within " + std::to_string(lim) + " bytes");
        len = static_cast<int>(static_cast<const char*>(nl) - p) + 1;
    });
    return rc < 0 ? rc : len;
}

int dcvc_y4m_write_header(char* dst, size_t cap, const dcvc_y4m_info* info)
{
    int len = -1;
    const int rc = dcvc::guarded([&] { len = write_header(dst, cap, info); });
    return rc < 0 ? rc : len;
}

}  // extern "C"
