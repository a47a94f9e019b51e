// rgb_cs.hip - 8-bit RGB pictures <-> the codec's fp16 NHWC picture tensor with a chosen colour matrix (BT.601, BT.709,
// BT.2020 non-constant luminance) and range (full, or limited: Y 16..235, C 16..240 scaled to the YUV bit depth): one kernel
// to x and one from x behind rgb_to_x / x_to_rgb (BT.709 / full range) and rgb_to_x_cs / x_to_rgb_cs.
//
// Reference at BT.709 / full range (a chain of torch ops on the GPU): test_video.py:87-122 get_src_frame with
// transforms.py:17-27 rgb2ycbcr (x.float() / 255, y = Kr r + Kg g + Kb b, cb / cr = 0.5 (b|r - y) / (1 - Kb|Kr) + 0.5,
// clamp(0, 1), .half(), - 0.5), test_video.py:55-64 get_distortion with transforms.py:53-66 ycbcr2rgb (x_hat + 0.5 in fp16,
// then in fp32 r = y + (2 - 2 Kr)(cr - 0.5), b = y + (2 - 2 Kb)(cb - 0.5), g = (y - Kr r - Kb b) / Kg, clamp(0, 1), .half(),
// then clamp(* 255, 0, 255) in fp16), :366-370 the writer (.round().byte()). torch's GPU true division by a CPU scalar is
// a * (1 / b) with the reciprocal rounded to fp32 (measured on MI355X over all 2^24 colours, DESIGN.md "RGB sources"); the
// kernels follow it, as that is what the reference computes on a GPU. The other matrices have no reference counterpart: the
// same op sequences with other constants and, in limited range, one multiply and one add (to x) or one subtract and one
// multiply (to RGB) per channel between the matrix and the fp16 rounding. DESIGN.md 20 has the definition; tests/colour_np.py
// restates it in numpy.
//
// Every torch op rounds on its own, so every step is one fp32 operation (the library builds with -ffp-contract=off: no
// v_fma) and every constant is the fp32 value of the Python double (expression) it stands for, computed on the host
// (colour_consts) and passed by value in the kernel argument: the constants are wave-uniform and sit in SGPRs. The range is
// a template switch, so the full-range kernels hold no extra operation.
//
// HBM-bound passes, one thread per 8 pixels of a row. A template switch picks 8- / 16-byte accesses where the layout
// allows them (packed HWC or planar CHW u8 input, packed x at ldx == 3, rows of a multiple of 8 pixels, aligned bases)
// and element accesses elsewhere (the slots of an 8-picture chunk at ldx = 24, odd-multiple-of-2 widths).
//
// 9..16-bit RGB (u16 samples, LSB-aligned, max_val = 2^b - 1) goes through a second kernel pair behind
// rgb16_to_x_cs / x_to_rgb16_cs with the same constants and the same per-pixel matrix code: to x, c = fp32(v) / fp32(max_val)
// is a correctly rounded division, as the 16-bit YUV reader's; from x, the distortion planes are fp32,
// clamp(fp32(t) * max_val, 0, max_val) with t = fp16(clamp(rgb, 0, 1)), as fp16 cannot hold a 10-bit sample, and the written
// sample is rint of that. The accesses are 16 bytes wide where the 8-bit pair's are 8.
#include "arith.h"
#include "picture_io.h"

namespace dcvc {

namespace {

constexpr int kThreads = kPictureThreads;
constexpr float kInv255 = 1.0f / 255.0f;                              // x.float() / 255.0

// what the two kernels read: the matrix (8 values) and the limited-range levels (6 values; unused in full range)
struct ColourConsts {
    float kr, kg, kb;               // fp32(Kr), fp32(Kg), fp32(Kb)
    float inv_1mkb, inv_1mkr;       // 1.0f / fp32(1 - Kb), 1.0f / fp32(1 - Kr)
    float inv_kg;                   // 1.0f / fp32(Kg)
    float c2m2kr, c2m2kb;           // fp32(2 - 2 Kr), fp32(2 - 2 Kb)
    float lo, ry, mid, rc;          // fp32(16 s / m), fp32(219 s / m), fp32(128 s / m), fp32(224 s / m)
    float iy, ic;                   // fp32(m / (219 s)), fp32(m / (224 s))
};

ColourConsts colour_consts(const ColourSpace& cs)
{
    static const double kK[3][3] = {{0.299, 0.587, 0.114}, {0.2126, 0.7152, 0.0722}, {0.2627, 0.6780, 0.0593}};
    const double Kr = kK[cs.matrix][0], Kg = kK[cs.matrix][1], Kb = kK[cs.matrix][2];
    ColourConsts c;
    c.kr = static_cast<float>(Kr); c.kg = static_cast<float>(Kg); c.kb = static_cast<float>(Kb);
    c.inv_1mkb = 1.0f / static_cast<float>(1.0 - Kb);
    c.inv_1mkr = 1.0f / static_cast<float>(1.0 - Kr);
    c.inv_kg = 1.0f / c.kg;
    c.c2m2kr = static_cast<float>(2 - 2 * Kr); c.c2m2kb = static_cast<float>(2 - 2 * Kb);
    // the levels of b-bit samples on x's scale v / (2^b - 1): one division in double each, then fp32
    const double s = static_cast<double>(1 << (cs.yuv_bit_depth - 8)), m = static_cast<double>((1 << cs.yuv_bit_depth) - 1);
    c.lo = static_cast<float>(16 * s / m); c.ry = static_cast<float>(219 * s / m);
    c.mid = static_cast<float>(128 * s / m); c.rc = static_cast<float>(224 * s / m);
    c.iy = static_cast<float>(m / (219 * s)); c.ic = static_cast<float>(m / (224 * s));
    return c;
}

// torch.clamp: NaN passes through
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one RGB pixel on the unit scale (sample / max_val) -> the three fp16 channels of x
template <bool LIMITED>
__device__ __forceinline__ void unit_to_x(const ColourConsts& k, float r, float g, float b, half_t* o)
{
    float y = (k.kr * r + k.kg * g) + k.kb * b;
    const float pb = (0.5f * (b - y)) * k.inv_1mkb;
    const float pr = (0.5f * (r - y)) * k.inv_1mkr;
    float cb, cr;
    if constexpr (LIMITED) {
        y = y * k.ry + k.lo;
        cb = pb * k.rc + k.mid;
        cr = pr * k.rc + k.mid;
    } else {
        cb = pb + 0.5f;
        cr = pr + 0.5f;
    }
    o[0] = to_half(static_cast<float>(to_half(clampf(y, 0.f, 1.f))) - 0.5f);
    o[1] = to_half(static_cast<float>(to_half(clampf(cb, 0.f, 1.f))) - 0.5f);
    o[2] = to_half(static_cast<float>(to_half(clampf(cr, 0.f, 1.f))) - 0.5f);
}

// 8 bits: x.float() / 255.0 is a multiply by the fp32 reciprocal
template <bool LIMITED>
__device__ __forceinline__ void pixel_to_x(const ColourConsts& k, unsigned r8, unsigned g8, unsigned b8, half_t* o)
{
    unit_to_x<LIMITED>(k, static_cast<float>(r8) * kInv255, static_cast<float>(g8) * kInv255, static_cast<float>(b8) * kInv255, o);
}

// 9..16 bits: a true division, correctly rounded (the library builds with -fno-fast-math), as the 16-bit YUV reader's
template <bool LIMITED>
__device__ __forceinline__ void pixel16_to_x(const ColourConsts& k, float maxv, unsigned r, unsigned g, unsigned b, half_t* o)
{
    unit_to_x<LIMITED>(k, static_cast<float>(r) / maxv, static_cast<float>(g) / maxv, static_cast<float>(b) / maxv, o);
}

// load modes of rgb_to_x
constexpr int kLoadScalar = 0, kLoadPacked = 1, kLoadPlanar = 2;

// one thread = 8 consecutive pixels of a row. LOAD: kLoadPacked (pixel stride 3, channel stride 1: 3 x 8-B loads),
// kLoadPlanar (pixel stride 1: one 8-B load per channel) or kLoadScalar (any strides). VEC_X: x at ldx == 3, 3 x 16-B
// stores. Vector modes need W % 8 == 0 and aligned rows (checked by the host).
template <int LOAD, bool VEC_X, bool LIMITED>
__global__ void __launch_bounds__(kThreads) rgb_to_x_kernel(const uint8_t* __restrict__ src, long long rs, long long ps,
                                                               long long cs, int H, int W, half_t* __restrict__ x, int ldx,
                                                               uint8_t* __restrict__ planar, const ColourConsts k)
{
    const unsigned wv = (W + 7) >> 3;
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;      // < 2^31 (picture_validate)
    if (i >= static_cast<unsigned>(H) * wv) return;
    const int h = static_cast<int>(i / wv), w0 = static_cast<int>(i - h * wv) * 8;
    const int n = min(8, W - w0);
    const uint8_t* row = src + h * rs + w0 * ps;
    uint8_t c[3][8];
    if constexpr (LOAD == kLoadPacked) {
        uint2 v[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) v[q] = reinterpret_cast<const uint2*>(row)[q];
        const uint8_t* bytes = reinterpret_cast<const uint8_t*>(v);
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int q = 0; q < 3; ++q) c[q][e] = bytes[3 * e + q];
    } else if constexpr (LOAD == kLoadPlanar) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const uint2 v = *reinterpret_cast<const uint2*>(row + q * cs);
            const uint8_t* bytes = reinterpret_cast<const uint8_t*>(&v);
#pragma unroll
            for (int e = 0; e < 8; ++e) c[q][e] = bytes[e];
        }
    } else {
        for (int e = 0; e < 8; ++e)
            for (int q = 0; q < 3; ++q) c[q][e] = e < n ? row[e * ps + q * cs] : 0;
    }
    if (planar) {
        const size_t plane = static_cast<size_t>(H) * W, o = static_cast<size_t>(h) * W + w0;
        if constexpr (LOAD != kLoadScalar) {
#pragma unroll
            for (int q = 0; q < 3; ++q) *reinterpret_cast<uint2*>(planar + q * plane + o) = *reinterpret_cast<const uint2*>(c[q]);
        } else {
            for (int e = 0; e < n; ++e)
                for (int q = 0; q < 3; ++q) planar[q * plane + o + e] = c[q][e];
        }
    }
    if (x) {
        half_t* o = x + (static_cast<size_t>(h) * W + w0) * ldx;
        if constexpr (VEC_X) {
            half8 v[3];
            half_t* hv = reinterpret_cast<half_t*>(v);
#pragma unroll
            for (int e = 0; e < 8; ++e) pixel_to_x<LIMITED>(k, c[0][e], c[1][e], c[2][e], hv + 3 * e);
#pragma unroll
            for (int q = 0; q < 3; ++q) reinterpret_cast<half8*>(o)[q] = v[q];
        } else {
            for (int e = 0; e < n; ++e) pixel_to_x<LIMITED>(k, c[0][e], c[1][e], c[2][e], o + e * ldx);
        }
    }
}

// one pixel of x_hat -> t = fp16(clamp(rgb, 0, 1)) of its three channels
template <bool LIMITED>
__device__ __forceinline__ void x_to_unit(const ColourConsts& k, const half_t* p, half_t* t)
{
    float y = static_cast<float>(to_half(static_cast<float>(p[0]) + 0.5f));              // x_hat + 0.5 (fp16)
    const float cb = static_cast<float>(to_half(static_cast<float>(p[1]) + 0.5f));
    const float cr = static_cast<float>(to_half(static_cast<float>(p[2]) + 0.5f));
    float pb, pr;
    if constexpr (LIMITED) {
        y = (y - k.lo) * k.iy;
        pb = (cb - k.mid) * k.ic;
        pr = (cr - k.mid) * k.ic;
    } else {
        pb = cb - 0.5f;
        pr = cr - 0.5f;
    }
    const float r = y + k.c2m2kr * pr;
    const float b = y + k.c2m2kb * pb;
    const float g = ((y - k.kr * r) - k.kb * b) * k.inv_kg;
    t[0] = to_half(clampf(r, 0.f, 1.f));                                                     // .to(fp16)
    t[1] = to_half(clampf(g, 0.f, 1.f));
    t[2] = to_half(clampf(b, 0.f, 1.f));
}

// one pixel of x_hat -> the three fp16 distortion samples (0..255)
template <bool LIMITED>
__device__ __forceinline__ void x_to_pixel(const ColourConsts& k, const half_t* p, half_t* o)
{
    half_t t[3];
    x_to_unit<LIMITED>(k, p, t);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float s = static_cast<float>(to_half(static_cast<float>(t[q]) * 255.0f));        // * 255 (fp16)
        o[q] = to_half(clampf(s, 0.f, 255.f));                                                  // clamp(0, 255), exact
    }
}

// 9..16 bits: the three fp32 distortion samples (0..max_val)
template <bool LIMITED>
__device__ __forceinline__ void x_to_pixel16(const ColourConsts& k, float maxv, const half_t* p, float* o)
{
    half_t t[3];
    x_to_unit<LIMITED>(k, p, t);
#pragma unroll
    for (int q = 0; q < 3; ++q) o[q] = clampf(static_cast<float>(t[q]) * maxv, 0.f, maxv);
}

// .round().byte(): half to even (the samples are in 0..255; NaN, which no clamp removes, is written as 0)
__device__ __forceinline__ uint8_t to_u8(half_t v)
{
    const float f = static_cast<float>(v);
    return f == f ? static_cast<uint8_t>(rintf(f)) : 0;
}

// one thread = 8 consecutive pixels of a row. VEC: row_pixels % 8 == 0, W % 8 == 0, aligned bases: 3 x 16-B loads,
// one 16-B store per fp16 plane, 3 x 8-B stores of packed u8.
template <bool VEC, bool LIMITED>
__global__ void __launch_bounds__(kThreads) x_to_rgb_kernel(const half_t* __restrict__ x, int row_pixels, int H, int W,
                                                               half_t* __restrict__ rgb16, uint8_t* __restrict__ rgb8,
                                                               const ColourConsts k)
{
    const unsigned wv = (W + 7) >> 3;
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;      // < 2^31 (picture_validate)
    if (i >= static_cast<unsigned>(H) * wv) return;
    const int h = static_cast<int>(i / wv), w0 = static_cast<int>(i - h * wv) * 8;
    const int n = min(8, W - w0);
    const half_t* p = x + (static_cast<size_t>(h) * row_pixels + w0) * 3;
    const size_t plane = static_cast<size_t>(H) * W, o = static_cast<size_t>(h) * W + w0;
    if constexpr (VEC) {
        half8 in[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) in[q] = reinterpret_cast<const half8*>(p)[q];
        const half_t* hin = reinterpret_cast<const half_t*>(in);
        half8 out[3];
        half_t* ho = reinterpret_cast<half_t*>(out);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            half_t t[3];
            x_to_pixel<LIMITED>(k, hin + 3 * e, t);
#pragma unroll
            for (int q = 0; q < 3; ++q) ho[q * 8 + e] = t[q];
        }
        if (rgb16) {
#pragma unroll
            for (int q = 0; q < 3; ++q) *reinterpret_cast<half8*>(rgb16 + q * plane + o) = out[q];
        }
        if (rgb8) {
            uint8_t b[24];
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int q = 0; q < 3; ++q) b[3 * e + q] = to_u8(ho[q * 8 + e]);
#pragma unroll
            for (int q = 0; q < 3; ++q) reinterpret_cast<uint2*>(rgb8 + o * 3)[q] = reinterpret_cast<const uint2*>(b)[q];
        }
    } else {
        for (int e = 0; e < n; ++e) {
            half_t t[3];
            x_to_pixel<LIMITED>(k, p + 3 * e, t);
            for (int q = 0; q < 3; ++q) {
                if (rgb16) rgb16[q * plane + o + e] = t[q];
                if (rgb8) rgb8[(o + e) * 3 + q] = to_u8(t[q]);
            }
        }
    }
}

// ---------------------------------------------------------------- 9..16 bits
// one thread = 8 consecutive pixels of a row of u16 samples. LOAD: kLoadPacked (3 x 16-B loads), kLoadPlanar (one 16-B load
// per channel) or kLoadScalar (any strides, element by element). VEC_X: x at ldx == 3, 3 x 16-B stores. Vector modes need
// W % 8 == 0 and 16-byte aligned rows (checked by the host); the planar copy then goes out in one 16-B store per channel.
template <int LOAD, bool VEC_X, bool LIMITED>
__global__ void __launch_bounds__(kThreads) rgb16_to_x_kernel(const uint16_t* __restrict__ src, long long rs, long long ps,
                                                                 long long cs, int H, int W, half_t* __restrict__ x, int ldx,
                                                                 uint16_t* __restrict__ planar, const ColourConsts k, float maxv)
{
    const unsigned wv = (W + 7) >> 3;
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;      // < 2^31 (picture_validate)
    if (i >= static_cast<unsigned>(H) * wv) return;
    const int h = static_cast<int>(i / wv), w0 = static_cast<int>(i - h * wv) * 8;
    const uint16_t* row = src + h * rs + w0 * ps;
    const size_t plane = static_cast<size_t>(H) * W, o = static_cast<size_t>(h) * W + w0;
    if constexpr (LOAD == kLoadScalar) {
        const int n = min(8, W - w0);
        for (int e = 0; e < n; ++e) {
            const unsigned r = row[e * ps], g = row[e * ps + cs], b = row[e * ps + 2 * cs];
            if (planar) {
                planar[o + e] = static_cast<uint16_t>(r);
                planar[plane + o + e] = static_cast<uint16_t>(g);
                planar[2 * plane + o + e] = static_cast<uint16_t>(b);
            }
            if (x) pixel16_to_x<LIMITED>(k, maxv, r, g, b, x + (o + e) * ldx);
        }
    } else {
        uint4 c[3];                                                // c[q]: the 8 samples of channel q
        uint16_t* cw = reinterpret_cast<uint16_t*>(c);
        if constexpr (LOAD == kLoadPacked) {
            uint4 v[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) v[q] = reinterpret_cast<const uint4*>(row)[q];
            const uint16_t* s = reinterpret_cast<const uint16_t*>(v);
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int q = 0; q < 3; ++q) cw[q * 8 + e] = s[3 * e + q];
        } else {
#pragma unroll
            for (int q = 0; q < 3; ++q) c[q] = *reinterpret_cast<const uint4*>(row + q * cs);
        }
        if (planar) {
#pragma unroll
            for (int q = 0; q < 3; ++q) *reinterpret_cast<uint4*>(planar + q * plane + o) = c[q];
        }
        if (x) {
            half_t* xo = x + o * ldx;
            if constexpr (VEC_X) {
                half8 v[3];
                half_t* hv = reinterpret_cast<half_t*>(v);
#pragma unroll
                for (int e = 0; e < 8; ++e) pixel16_to_x<LIMITED>(k, maxv, cw[e], cw[8 + e], cw[16 + e], hv + 3 * e);
#pragma unroll
                for (int q = 0; q < 3; ++q) reinterpret_cast<half8*>(xo)[q] = v[q];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) pixel16_to_x<LIMITED>(k, maxv, cw[e], cw[8 + e], cw[16 + e], xo + e * ldx);
            }
        }
    }
}

// .round() to u16: half to even (the samples are in 0..max_val; NaN, which no clamp removes, is written as 0)
__device__ __forceinline__ uint16_t to_u16(float f) { return f == f ? static_cast<uint16_t>(rintf(f)) : 0; }

// one thread = 8 consecutive pixels of a row. VEC: row_pixels % 8 == 0, W % 8 == 0, aligned bases: 3 x 16-B loads, two 16-B
// stores per fp32 plane, 3 x 16-B stores of packed u16.
template <bool VEC, bool LIMITED>
__global__ void __launch_bounds__(kThreads) x_to_rgb16_kernel(const half_t* __restrict__ x, int row_pixels, int H, int W,
                                                                 float* __restrict__ dist, uint16_t* __restrict__ out,
                                                                 const ColourConsts k, float maxv)
{
    const unsigned wv = (W + 7) >> 3;
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;      // < 2^31 (picture_validate)
    if (i >= static_cast<unsigned>(H) * wv) return;
    const int h = static_cast<int>(i / wv), w0 = static_cast<int>(i - h * wv) * 8;
    const half_t* p = x + (static_cast<size_t>(h) * row_pixels + w0) * 3;
    const size_t plane = static_cast<size_t>(H) * W, o = static_cast<size_t>(h) * W + w0;
    if constexpr (VEC) {
        half8 in[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) in[q] = reinterpret_cast<const half8*>(p)[q];
        const half_t* hin = reinterpret_cast<const half_t*>(in);
        float4 d[3][2];                                            // d[q]: the 8 distortion samples of channel q
        float* df = reinterpret_cast<float*>(d);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float t[3];
            x_to_pixel16<LIMITED>(k, maxv, hin + 3 * e, t);
#pragma unroll
            for (int q = 0; q < 3; ++q) df[q * 8 + e] = t[q];
        }
        if (dist) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                reinterpret_cast<float4*>(dist + q * plane + o)[0] = d[q][0];
                reinterpret_cast<float4*>(dist + q * plane + o)[1] = d[q][1];
            }
        }
        if (out) {
            uint4 v[3];
            uint16_t* s = reinterpret_cast<uint16_t*>(v);
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int q = 0; q < 3; ++q) s[3 * e + q] = to_u16(df[q * 8 + e]);
#pragma unroll
            for (int q = 0; q < 3; ++q) reinterpret_cast<uint4*>(out + o * 3)[q] = v[q];
        }
    } else {
        const int n = min(8, W - w0);
        for (int e = 0; e < n; ++e) {
            float t[3];
            x_to_pixel16<LIMITED>(k, maxv, p + 3 * e, t);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if (dist) dist[q * plane + o + e] = t[q];
                if (out) out[(o + e) * 3 + q] = to_u16(t[q]);
            }
        }
    }
}

void colour_validate(const ColourSpace& cs, const char* what)
{
    if (cs.matrix != kMatrixBt601 && cs.matrix != kMatrixBt709 && cs.matrix != kMatrixBt2020) {
        throw std::invalid_argument(std::string(what) + ": unknown colour matrix " + std::to_string(cs.matrix));
    }
    if (cs.range != kRangeFull && cs.range != kRangeLimited) {
        throw std::invalid_argument(std::string(what) + ": unknown colour range " + std::to_string(cs.range));
    }
    if (cs.yuv_bit_depth < 8 || cs.yuv_bit_depth > 16) {
        throw std::invalid_argument(std::string(what) + ": the YUV bit depth must be in 8..16, got " + std::to_string(cs.yuv_bit_depth));
    }
}

template <int LOAD, bool VEC_X>
void launch_to_x(const RgbToXDesc& d, bool limited, const ColourConsts& k, hipStream_t stream)
{
    const dim3 grid(grid_of(d.H, d.W)), block(kThreads);
    if (limited) {
        hipLaunchKernelGGL((rgb_to_x_kernel<LOAD, VEC_X, true>), grid, block, 0, stream, d.src, d.row_stride, d.pixel_stride,
                           d.channel_stride, d.H, d.W, d.x, d.ldx, d.planar, k);
    } else {
        hipLaunchKernelGGL((rgb_to_x_kernel<LOAD, VEC_X, false>), grid, block, 0, stream, d.src, d.row_stride, d.pixel_stride,
                           d.channel_stride, d.H, d.W, d.x, d.ldx, d.planar, k);
    }
}

// the three (stride, extent) pairs must not overlap: sorted by stride, each stride covers the previous dimension
template <typename Desc>
void stride_check(const Desc& d, const std::string& what)
{
    long long st[3] = {d.channel_stride, d.pixel_stride, d.row_stride}, ex[3] = {3, d.W, d.H};
    for (int q = 0; q < 3; ++q) {
        if (st[q] <= 0) throw std::invalid_argument(what + ": the source strides must be positive");
    }
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b)
            if (st[b] < st[a]) { std::swap(st[a], st[b]); std::swap(ex[a], ex[b]); }
    if (st[1] < st[0] * ex[0] || st[2] < st[1] * ex[1]) {
        throw std::invalid_argument(what + ": source strides too small (row " + std::to_string(d.row_stride) + ", pixel " +
                                    std::to_string(d.pixel_stride) + ", channel " + std::to_string(d.channel_stride) +
                                    " for " + std::to_string(d.W) + "x" + std::to_string(d.H) + ")");
    }
}

// what: the entry's name, the prefix of its refusals
void to_x(const RgbToXDesc& d, const ColourSpace& cs, const std::string& what, hipStream_t stream)
{
    picture_validate(d.H, d.W, what.c_str());
    colour_validate(cs, what.c_str());
    if (d.src == nullptr) throw std::invalid_argument(what + ": no source picture");
    if (d.x == nullptr && d.planar == nullptr) throw std::invalid_argument(what + ": neither x nor the planar copy requested");
    if (d.x != nullptr && d.ldx < 3) throw std::invalid_argument(what + ": the pixel stride of x must be >= 3");
    stride_check(d, what);
    const bool rows8 = d.W % 8 == 0 && d.row_stride % 8 == 0 && aligned(d.src, 8) && (d.planar == nullptr || aligned(d.planar, 8));
    int load = kLoadScalar;
    if (rows8 && d.pixel_stride == 3 && d.channel_stride == 1) load = kLoadPacked;
    else if (rows8 && d.pixel_stride == 1 && d.channel_stride % 8 == 0) load = kLoadPlanar;
    const bool vec_x = d.x != nullptr && load != kLoadScalar && d.ldx == 3 && aligned(d.x, 16);
    const bool limited = cs.range == kRangeLimited;
    const ColourConsts k = colour_consts(cs);
    if (load == kLoadPacked && vec_x) launch_to_x<kLoadPacked, true>(d, limited, k, stream);
    else if (load == kLoadPacked) launch_to_x<kLoadPacked, false>(d, limited, k, stream);
    else if (load == kLoadPlanar && vec_x) launch_to_x<kLoadPlanar, true>(d, limited, k, stream);
    else if (load == kLoadPlanar) launch_to_x<kLoadPlanar, false>(d, limited, k, stream);
    else launch_to_x<kLoadScalar, false>(d, limited, k, stream);
    hip_check(hipGetLastError(), (what + " launch").c_str());
}

void from_x(const half_t* x, int row_pixels, int H, int W, half_t* rgb16, uint8_t* rgb8, const ColourSpace& cs, const std::string& what,
            hipStream_t stream)
{
    picture_validate(H, W, what.c_str());
    colour_validate(cs, what.c_str());
    if (x == nullptr) throw std::invalid_argument(what + ": no x_hat");
    if (row_pixels < W) throw std::invalid_argument(what + ": the rows of x_hat are shorter than the picture");
    const bool vec = row_pixels % 8 == 0 && W % 8 == 0 && aligned(x, 16) && (rgb16 == nullptr || aligned(rgb16, 16)) &&
                     (rgb8 == nullptr || aligned(rgb8, 8));
    if (rgb16 == nullptr && rgb8 == nullptr) return;
    const bool limited = cs.range == kRangeLimited;
    const ColourConsts k = colour_consts(cs);
    const dim3 grid(grid_of(H, W)), block(kThreads);
    if (vec && limited) hipLaunchKernelGGL((x_to_rgb_kernel<true, true>), grid, block, 0, stream, x, row_pixels, H, W, rgb16, rgb8, k);
    else if (vec) hipLaunchKernelGGL((x_to_rgb_kernel<true, false>), grid, block, 0, stream, x, row_pixels, H, W, rgb16, rgb8, k);
    else if (limited) hipLaunchKernelGGL((x_to_rgb_kernel<false, true>), grid, block, 0, stream, x, row_pixels, H, W, rgb16, rgb8, k);
    else hipLaunchKernelGGL((x_to_rgb_kernel<false, false>), grid, block, 0, stream, x, row_pixels, H, W, rgb16, rgb8, k);
    hip_check(hipGetLastError(), (what + " launch").c_str());
}

float depth_max_val(int bit_depth, const std::string& what)
{
    if (bit_depth < 9 || bit_depth > 16) {
        throw std::invalid_argument(what + ": the bit depth must be in 9..16 (8-bit pictures go through the u8 entry points), got " +
                                    std::to_string(bit_depth));
    }
    return static_cast<float>((1 << bit_depth) - 1);      // exact in fp32
}

template <int LOAD, bool VEC_X>
void launch_to_x16(const Rgb16ToXDesc& d, bool limited, const ColourConsts& k, float maxv, hipStream_t stream)
{
    const dim3 grid(grid_of(d.H, d.W)), block(kThreads);
    if (limited) {
        hipLaunchKernelGGL((rgb16_to_x_kernel<LOAD, VEC_X, true>), grid, block, 0, stream, d.src, d.row_stride, d.pixel_stride,
                           d.channel_stride, d.H, d.W, d.x, d.ldx, d.planar, k, maxv);
    } else {
        hipLaunchKernelGGL((rgb16_to_x_kernel<LOAD, VEC_X, false>), grid, block, 0, stream, d.src, d.row_stride, d.pixel_stride,
                           d.channel_stride, d.H, d.W, d.x, d.ldx, d.planar, k, maxv);
    }
}

void to_x16(const Rgb16ToXDesc& d, const ColourSpace& cs, const std::string& what, hipStream_t stream)
{
    picture_validate(d.H, d.W, what.c_str());
    const float maxv = depth_max_val(d.bit_depth, what);
    colour_validate(cs, what.c_str());
    if (d.src == nullptr) throw std::invalid_argument(what + ": no source picture");
    if (d.x == nullptr && d.planar == nullptr) throw std::invalid_argument(what + ": neither x nor the planar copy requested");
    if (d.x != nullptr && d.ldx < 3) throw std::invalid_argument(what + ": the pixel stride of x must be >= 3");
    stride_check(d, what);
    // strides in samples: 8 samples are the 16 bytes of one access
    const bool rows8 = d.W % 8 == 0 && d.row_stride % 8 == 0 && aligned(d.src, 16) && (d.planar == nullptr || aligned(d.planar, 16));
    int load = kLoadScalar;
    if (rows8 && d.pixel_stride == 3 && d.channel_stride == 1) load = kLoadPacked;
    else if (rows8 && d.pixel_stride == 1 && d.channel_stride % 8 == 0) load = kLoadPlanar;
    const bool vec_x = d.x != nullptr && load != kLoadScalar && d.ldx == 3 && aligned(d.x, 16);
    const bool limited = cs.range == kRangeLimited;
    const ColourConsts k = colour_consts(cs);
    if (load == kLoadPacked && vec_x) launch_to_x16<kLoadPacked, true>(d, limited, k, maxv, stream);
    else if (load == kLoadPacked) launch_to_x16<kLoadPacked, false>(d, limited, k, maxv, stream);
    else if (load == kLoadPlanar && vec_x) launch_to_x16<kLoadPlanar, true>(d, limited, k, maxv, stream);
    else if (load == kLoadPlanar) launch_to_x16<kLoadPlanar, false>(d, limited, k, maxv, stream);
    else launch_to_x16<kLoadScalar, false>(d, limited, k, maxv, stream);
    hip_check(hipGetLastError(), (what + " launch").c_str());
}

void from_x16(const half_t* x, int row_pixels, int H, int W, int bit_depth, float* dist, uint16_t* out, const ColourSpace& cs,
              const std::string& what, hipStream_t stream)
{
    picture_validate(H, W, what.c_str());
    const float maxv = depth_max_val(bit_depth, what);
    colour_validate(cs, what.c_str());
    if (x == nullptr) throw std::invalid_argument(what + ": no x_hat");
    if (dist == nullptr && out == nullptr) throw std::invalid_argument(what + ": neither the distortion planes nor the samples requested");
    if (row_pixels < W) throw std::invalid_argument(what + ": the rows of x_hat are shorter than the picture");
    const bool vec = row_pixels % 8 == 0 && W % 8 == 0 && aligned(x, 16) && (dist == nullptr || aligned(dist, 16)) &&
                     (out == nullptr || aligned(out, 16));
    const bool limited = cs.range == kRangeLimited;
    const ColourConsts k = colour_consts(cs);
    const dim3 grid(grid_of(H, W)), block(kThreads);
    if (vec && limited) hipLaunchKernelGGL((x_to_rgb16_kernel<true, true>), grid, block, 0, stream, x, row_pixels, H, W, dist, out, k, maxv);
    else if (vec) hipLaunchKernelGGL((x_to_rgb16_kernel<true, false>), grid, block, 0, stream, x, row_pixels, H, W, dist, out, k, maxv);
    else if (limited) hipLaunchKernelGGL((x_to_rgb16_kernel<false, true>), grid, block, 0, stream, x, row_pixels, H, W, dist, out, k, maxv);
    else hipLaunchKernelGGL((x_to_rgb16_kernel<false, false>), grid, block, 0, stream, x, row_pixels, H, W, dist, out, k, maxv);
    hip_check(hipGetLastError(), (what + " launch").c_str());
}

}  // namespace

void rgb_to_x(const RgbToXDesc& d, hipStream_t stream) { to_x(d, ColourSpace{}, "rgb_to_x", stream); }

void rgb_to_x_cs(const RgbToXDesc& d, const ColourSpace& cs, hipStream_t stream) { to_x(d, cs, "rgb_to_x_cs", stream); }

void x_to_rgb(const half_t* x, int row_pixels, int H, int W, half_t* rgb16, uint8_t* rgb8, hipStream_t stream)
{
    from_x(x, row_pixels, H, W, rgb16, rgb8, ColourSpace{}, "x_to_rgb", stream);
}

void x_to_rgb_cs(const half_t* x, int row_pixels, int H, int W, half_t* rgb16, uint8_t* rgb8, const ColourSpace& cs, hipStream_t stream)
{
    from_x(x, row_pixels, H, W, rgb16, rgb8, cs, "x_to_rgb_cs", stream);
}

void rgb16_to_x_cs(const Rgb16ToXDesc& d, const ColourSpace& cs, hipStream_t stream) { to_x16(d, cs, "rgb16_to_x_cs", stream); }

void x_to_rgb16_cs(const half_t* x, int row_pixels, int H, int W, int bit_depth, float* dist32, uint16_t* rgb16u, const ColourSpace& cs,
                   hipStream_t stream)
{
    from_x16(x, row_pixels, H, W, bit_depth, dist32, rgb16u, cs, "x_to_rgb16_cs", stream);
}

}  // namespace dcvc
