// rgb_io.hip - 8-bit RGB pictures <-> the codec's fp16 NHWC picture tensor (BT.709), and the fp64 sum of squared differences
// behind the RGB PSNR, on the GPU.
//
// Reference (a chain of torch ops on the GPU): test_video.py:87-122 get_src_frame with transforms.py:17-27 rgb2ycbcr
// (x.float() / 255, y = Kr r + Kg g + Kb b, cb / cr = 0.5 (b|r - y) / (1 - Kb|Kr) + 0.5, clamp(0, 1), .half(), - 0.5),
// test_video.py:55-64 get_distortion with transforms.py:53-66 ycbcr2rgb (x_hat + 0.5 in fp16, then in fp32
// r = y + (2 - 2 Kr)(cr - 0.5), b = y + (2 - 2 Kb)(cb - 0.5), g = (y - Kr r - Kb b) / Kg, clamp(0, 1), .half(), then
// clamp(* 255, 0, 255) in fp16), :366-370 the writer (.round().byte()), metrics.py:10-24 calc_psnr (fp64 mean square).
//
// Every torch op rounds on its own, so every step here is one fp32 operation (the library builds with -ffp-contract=off:
// no v_fma), and each constant is the fp32 value of the Python double (expression) it stands for. torch's GPU true
// division by a CPU scalar is a * (1 / b) with the reciprocal rounded to fp32 (measured on MI355X over all 2^24 colours,
// DESIGN.md "RGB sources"); the kernels follow it, as that is what the reference computes on a GPU.
//
// HBM-bound passes, one thread per 8 pixels of a row. A template switch picks 8- / 16-byte accesses where the layout
// allows them (packed HWC or planar CHW u8 input, packed x at ldx == 3, rows of a multiple of 8 pixels, aligned bases)
// and element accesses elsewhere (the slots of an 8-picture chunk at ldx = 24, odd-multiple-of-2 widths). The sum of
// squares writes one fp64 partial per workgroup and reduces them in a second launch in a fixed order: no atomics, the
// result is bitwise reproducible and independent of how many planes one call covers.
#include "arith.h"
#include "ops.h"

namespace dcvc {

namespace {

constexpr double kKr = 0.2126, kKg = 0.7152, kKb = 0.0722;      // ITU-R BT.709 (transforms.py:10-14)
constexpr float fKr = static_cast<float>(kKr), fKg = static_cast<float>(kKg), fKb = static_cast<float>(kKb);
constexpr float kInv255 = 1.0f / 255.0f;                              // x.float() / 255.0
constexpr float kInv1mKb = 1.0f / static_cast<float>(1.0 - kKb);     // ... / (1 - Kb)
constexpr float kInv1mKr = 1.0f / static_cast<float>(1.0 - kKr);
constexpr float kInvKg = 1.0f / fKg;                                  // ... / Kg
constexpr float k2m2Kr = static_cast<float>(2 - 2 * kKr), k2m2Kb = static_cast<float>(2 - 2 * kKb);
constexpr int kThreads = 256;
constexpr int kSsePartials = 1024;       // most workgroups per plane of the sum of squares (a function of H, W alone)

// torch.clamp: NaN passes through
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// rgb2ycbcr of one pixel -> the three fp16 channels of x
__device__ __forceinline__ void pixel_to_x(unsigned r8, unsigned g8, unsigned b8, half_t* o)
{
    const float r = static_cast<float>(r8) * kInv255, g = static_cast<float>(g8) * kInv255, b = static_cast<float>(b8) * kInv255;
    const float y = (fKr * r + fKg * g) + fKb * b;
    const float cb = (0.5f * (b - y)) * kInv1mKb + 0.5f;
    const float cr = (0.5f * (r - y)) * kInv1mKr + 0.5f;
    o[0] = to_half(static_cast<float>(to_half(clampf(y, 0.f, 1.f))) - 0.5f);
    o[1] = to_half(static_cast<float>(to_half(clampf(cb, 0.f, 1.f))) - 0.5f);
    o[2] = to_half(static_cast<float>(to_half(clampf(cr, 0.f, 1.f))) - 0.5f);
}

// load modes of rgb_to_x
constexpr int kLoadScalar = 0, kLoadPacked = 1, kLoadPlanar = 2;

// one thread = 8 consecutive pixels of a row. LOAD: kLoadPacked (pixel stride 3, channel stride 1: 3 x 8-B loads),
// kLoadPlanar (pixel stride 1: one 8-B load per channel) or kLoadScalar (any strides). VEC_X: x at ldx == 3, 3 x 16-B
// stores. Vector modes need W % 8 == 0 and aligned rows (checked by the host).
template <int LOAD, bool VEC_X>
__global__ void __launch_bounds__(kThreads) rgb_to_x_kernel(const uint8_t* __restrict__ src, long long rs, long long ps,
                                                            long long cs, int H, int W, half_t* __restrict__ x, int ldx,
                                                            uint8_t* __restrict__ planar)
{
    const unsigned wv = (W + 7) >> 3;
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;      // < 2^31 (rgb_validate)
    if (i >= static_cast<unsigned>(H) * wv) return;
    const int h = static_cast<int>(i / wv), w0 = static_cast<int>(i - h * wv) * 8;
    const int n = min(8, W - w0);
    const uint8_t* row = src + h * rs + w0 * ps;
    uint8_t c[3][8];
    if constexpr (LOAD == kLoadPacked) {
        uint2 v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = reinterpret_cast<const uint2*>(row)[k];
        const uint8_t* bytes = reinterpret_cast<const uint8_t*>(v);
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k][e] = bytes[3 * e + k];
    } else if constexpr (LOAD == kLoadPlanar) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint2 v = *reinterpret_cast<const uint2*>(row + k * cs);
            const uint8_t* bytes = reinterpret_cast<const uint8_t*>(&v);
#pragma unroll
            for (int e = 0; e < 8; ++e) c[k][e] = bytes[e];
        }
    } else {
        for (int e = 0; e < 8; ++e)
            for (int k = 0; k < 3; ++k) c[k][e] = e < n ? row[e * ps + k * cs] : 0;
    }
    if (planar) {
        const size_t plane = static_cast<size_t>(H) * W, o = static_cast<size_t>(h) * W + w0;
        if constexpr (LOAD != kLoadScalar) {
#pragma unroll
            for (int k = 0; k < 3; ++k) *reinterpret_cast<uint2*>(planar + k * plane + o) = *reinterpret_cast<const uint2*>(c[k]);
        } else {
            for (int e = 0; e < n; ++e)
                for (int k = 0; k < 3; ++k) planar[k * plane + o + e] = c[k][e];
        }
    }
    if (x) {
        half_t* o = x + (static_cast<size_t>(h) * W + w0) * ldx;
        if constexpr (VEC_X) {
            half8 v[3];
            half_t* hv = reinterpret_cast<half_t*>(v);
#pragma unroll
            for (int e = 0; e < 8; ++e) pixel_to_x(c[0][e], c[1][e], c[2][e], hv + 3 * e);
#pragma unroll
            for (int k = 0; k < 3; ++k) reinterpret_cast<half8*>(o)[k] = v[k];
        } else {
            for (int e = 0; e < n; ++e) pixel_to_x(c[0][e], c[1][e], c[2][e], o + e * ldx);
        }
    }
}

// ycbcr2rgb of one pixel of x_hat -> the three fp16 distortion samples (0..255)
__device__ __forceinline__ void x_to_pixel(const half_t* p, half_t* o)
{
    const float y = static_cast<float>(to_half(static_cast<float>(p[0]) + 0.5f));        // x_hat + 0.5 (fp16)
    const float cb = static_cast<float>(to_half(static_cast<float>(p[1]) + 0.5f));
    const float cr = static_cast<float>(to_half(static_cast<float>(p[2]) + 0.5f));
    const float r = y + k2m2Kr * (cr - 0.5f);
    const float b = y + k2m2Kb * (cb - 0.5f);
    const float g = ((y - fKr * r) - fKb * b) * kInvKg;
    const float rgb[3] = {r, g, b};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const half_t t = to_half(clampf(rgb[k], 0.f, 1.f));                                  // .to(fp16)
        const float s = static_cast<float>(to_half(static_cast<float>(t) * 255.0f));           // * 255 (fp16)
        o[k] = to_half(clampf(s, 0.f, 255.f));                                                  // clamp(0, 255), exact
    }
}

// .round().byte(): half to even (the samples are in 0..255; NaN, which no clamp removes, is written as 0)
__device__ __forceinline__ uint8_t to_u8(half_t v)
{
    const float f = static_cast<float>(v);
    return f == f ? static_cast<uint8_t>(rintf(f)) : 0;
}

// one thread = 8 consecutive pixels of a row. VEC: row_pixels % 8 == 0, W % 8 == 0, aligned bases: 3 x 16-B loads,
// one 16-B store per fp16 plane, 3 x 8-B stores of packed u8.
template <bool VEC>
__global__ void __launch_bounds__(kThreads) x_to_rgb_kernel(const half_t* __restrict__ x, int row_pixels, int H, int W,
                                                            half_t* __restrict__ rgb16, uint8_t* __restrict__ rgb8)
{
    const unsigned wv = (W + 7) >> 3;
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;      // < 2^31 (rgb_validate)
    if (i >= static_cast<unsigned>(H) * wv) return;
    const int h = static_cast<int>(i / wv), w0 = static_cast<int>(i - h * wv) * 8;
    const int n = min(8, W - w0);
    const half_t* p = x + (static_cast<size_t>(h) * row_pixels + w0) * 3;
    const size_t plane = static_cast<size_t>(H) * W, o = static_cast<size_t>(h) * W + w0;
    if constexpr (VEC) {
        half8 in[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) in[k] = reinterpret_cast<const half8*>(p)[k];
        const half_t* hin = reinterpret_cast<const half_t*>(in);
        half8 out[3];
        half_t* ho = reinterpret_cast<half_t*>(out);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            half_t t[3];
            x_to_pixel(hin + 3 * e, t);
#pragma unroll
            for (int k = 0; k < 3; ++k) ho[k * 8 + e] = t[k];
        }
        if (rgb16) {
#pragma unroll
            for (int k = 0; k < 3; ++k) *reinterpret_cast<half8*>(rgb16 + k * plane + o) = out[k];
        }
        if (rgb8) {
            uint8_t b[24];
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int k = 0; k < 3; ++k) b[3 * e + k] = to_u8(ho[k * 8 + e]);
#pragma unroll
            for (int k = 0; k < 3; ++k) reinterpret_cast<uint2*>(rgb8 + o * 3)[k] = reinterpret_cast<const uint2*>(b)[k];
        }
    } else {
        for (int e = 0; e < n; ++e) {
            half_t t[3];
            x_to_pixel(p + 3 * e, t);
            for (int k = 0; k < 3; ++k) {
                if (rgb16) rgb16[k * plane + o + e] = t[k];
                if (rgb8) rgb8[(o + e) * 3 + k] = to_u8(t[k]);
            }
        }
    }
}

__device__ __forceinline__ double sample(uint8_t v) { return static_cast<double>(v); }
__device__ __forceinline__ double sample(half_t v) { return static_cast<double>(static_cast<float>(v)); }
__device__ __forceinline__ double sample(uint16_t v) { return static_cast<double>(v); }
__device__ __forceinline__ double sample(float v) { return static_cast<double>(v); }

// 8 samples in one access (u8: 8 B; fp16, u16: 16 B) or two (fp32: 2 x 16 B)
template <typename T> struct Vec8 { T v[8]; };
template <typename T> __device__ __forceinline__ Vec8<T> load8(const T* p)
{
    Vec8<T> r;
    if constexpr (sizeof(T) == 1) {
        *reinterpret_cast<uint2*>(r.v) = *reinterpret_cast<const uint2*>(p);
    } else if constexpr (sizeof(T) == 2) {
        *reinterpret_cast<uint4*>(r.v) = *reinterpret_cast<const uint4*>(p);
    } else {
        reinterpret_cast<uint4*>(r.v)[0] = reinterpret_cast<const uint4*>(p)[0];
        reinterpret_cast<uint4*>(r.v)[1] = reinterpret_cast<const uint4*>(p)[1];
    }
    return r;
}

// fixed-order sum over the workgroup (256 threads = 4 waves); valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* scratch)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
        for (int k = 0; k < kThreads / 64; ++k) s += scratch[k];
    }
    return s;
}

// partial[plane][blockIdx.x]: the squared differences of 8-sample row pieces blockIdx.x, + gridDim.x, ... of one plane
template <typename TA, typename TB, bool VEC>
__global__ void __launch_bounds__(kThreads) sse_partial_kernel(const TA* __restrict__ a, const TB* __restrict__ b, int H, int W,
                                                               long long row_stride, long long plane_stride,
                                                               double* __restrict__ partial)
{
    __shared__ double scratch[kThreads / 64];
    const unsigned wv = (W + 7) >> 3;
    const unsigned pieces = static_cast<unsigned>(H) * wv;       // < 2^31 (sse_validate)
    const long long base = static_cast<long long>(blockIdx.y) * plane_stride;
    double s = 0.0;
    for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < pieces; i += gridDim.x * kThreads) {
        const int h = static_cast<int>(i / wv), w0 = static_cast<int>(i - h * wv) * 8;
        const long long off = base + h * row_stride + w0;
        if constexpr (VEC) {
            const Vec8<TA> va = load8(a + off);
            const Vec8<TB> vb = load8(b + off);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const double d = sample(va.v[e]) - sample(vb.v[e]);
                s += d * d;
            }
        } else {
            const int n = min(8, W - w0);
            for (int e = 0; e < n; ++e) {
                const double d = sample(a[off + e]) - sample(b[off + e]);
                s += d * d;
            }
        }
    }
    const double t = block_sum(s, scratch);
    if (threadIdx.x == 0) partial[static_cast<long long>(blockIdx.y) * gridDim.x + blockIdx.x] = t;
}

// out[plane] = the sum of that plane's `parts` partials, in a fixed order
__global__ void __launch_bounds__(kThreads) sse_final_kernel(const double* __restrict__ partial, int parts, double* __restrict__ out)
{
    __shared__ double scratch[kThreads / 64];
    const double* q = partial + static_cast<long long>(blockIdx.x) * parts;
    double s = 0.0;
    for (int k = threadIdx.x; k < parts; k += kThreads) s += q[k];
    const double t = block_sum(s, scratch);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

unsigned grid_of(int H, int W)
{
    const long long n = static_cast<long long>(H) * ((W + 7) / 8);
    return static_cast<unsigned>((n + kThreads - 1) / kThreads);
}

int sse_parts(int H, int W)
{
    const long long pieces = static_cast<long long>(H) * ((W + 7) / 8);
    return static_cast<int>(std::min<long long>(kSsePartials, (pieces + kThreads - 1) / kThreads));
}

template <typename TA, typename TB>
void launch_sse(const TA* a, const TB* b, const SseDesc& d, double* partial, int parts, hipStream_t stream)
{
    // 8-sample pieces: one 8-B (u8) or 16-B (fp16, u16) load, or two 16-B loads (fp32), per operand
    const bool vec = d.W % 8 == 0 && d.row_stride % 8 == 0 && (d.n_planes == 1 || d.plane_stride % 8 == 0) &&
                     aligned(a, std::min<size_t>(16, 8 * sizeof(TA))) && aligned(b, std::min<size_t>(16, 8 * sizeof(TB)));
    const dim3 grid(static_cast<unsigned>(parts), static_cast<unsigned>(d.n_planes));
    if (vec) {
        hipLaunchKernelGGL((sse_partial_kernel<TA, TB, true>), grid, dim3(kThreads), 0, stream, a, b, d.H, d.W,
                           static_cast<long long>(d.row_stride), d.plane_stride, partial);
    } else {
        hipLaunchKernelGGL((sse_partial_kernel<TA, TB, false>), grid, dim3(kThreads), 0, stream, a, b, d.H, d.W,
                           static_cast<long long>(d.row_stride), d.plane_stride, partial);
    }
}

template <typename TA>
void launch_sse_b(const TA* a, const SseDesc& d, double* partial, int parts, hipStream_t stream)
{
    switch (d.rec_dtype) {
    case kSampleU8: launch_sse(a, static_cast<const uint8_t*>(d.rec), d, partial, parts, stream); break;
    case kSampleF16: launch_sse(a, static_cast<const half_t*>(d.rec), d, partial, parts, stream); break;
    case kSampleU16: launch_sse(a, static_cast<const uint16_t*>(d.rec), d, partial, parts, stream); break;
    default: launch_sse(a, static_cast<const float*>(d.rec), d, partial, parts, stream); break;
    }
}

}  // namespace

void rgb_validate(int H, int W, const char* what)
{
    if (H <= 0 || W <= 0 || (H & 1) || (W & 1)) {
        throw std::invalid_argument(std::string(what) + ": the picture sides must be positive and even, got " +
                                    std::to_string(W) + "x" + std::to_string(H));
    }
    // one thread per 8 pixels of a row, 32-bit thread indices (addresses are 64-bit)
    if (static_cast<long long>(H) * ((W + 7) / 8) + kThreads > (1LL << 31)) throw std::invalid_argument(std::string(what) + ": picture too large");
}

void rgb_to_x(const RgbToXDesc& d, hipStream_t stream)
{
    rgb_validate(d.H, d.W, "rgb_to_x");
    if (d.src == nullptr) throw std::invalid_argument("rgb_to_x: no source picture");
    if (d.x == nullptr && d.planar == nullptr) throw std::invalid_argument("rgb_to_x: neither x nor the planar copy requested");
    if (d.x != nullptr && d.ldx < 3) throw std::invalid_argument("rgb_to_x: the pixel stride of x must be >= 3");
    // the three (stride, extent) pairs must not overlap: sorted by stride, each stride covers the previous dimension
    long long st[3] = {d.channel_stride, d.pixel_stride, d.row_stride}, ex[3] = {3, d.W, d.H};
    for (int k = 0; k < 3; ++k) {
        if (st[k] <= 0) throw std::invalid_argument("rgb_to_x: the source strides must be positive");
    }
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b)
            if (st[b] < st[a]) { std::swap(st[a], st[b]); std::swap(ex[a], ex[b]); }
    if (st[1] < st[0] * ex[0] || st[2] < st[1] * ex[1]) {
        throw std::invalid_argument("rgb_to_x: source strides too small (row " + std::to_string(d.row_stride) + ", pixel " +
                                    std::to_string(d.pixel_stride) + ", channel " + std::to_string(d.channel_stride) +
                                    " for " + std::to_string(d.W) + "x" + std::to_string(d.H) + ")");
    }
    const bool rows8 = d.W % 8 == 0 && d.row_stride % 8 == 0 && aligned(d.src, 8) && (d.planar == nullptr || aligned(d.planar, 8));
    int load = kLoadScalar;
    if (rows8 && d.pixel_stride == 3 && d.channel_stride == 1) load = kLoadPacked;
    else if (rows8 && d.pixel_stride == 1 && d.channel_stride % 8 == 0) load = kLoadPlanar;
    const bool vec_x = d.x != nullptr && load != kLoadScalar && d.ldx == 3 && aligned(d.x, 16);
    const dim3 grid(grid_of(d.H, d.W)), block(kThreads);
#define RGB_TO_X_ARGS stream, d.src, d.row_stride, d.pixel_stride, d.channel_stride, d.H, d.W, d.x, d.ldx, d.planar
    if (load == kLoadPacked && vec_x) hipLaunchKernelGGL((rgb_to_x_kernel<kLoadPacked, true>), grid, block, 0, RGB_TO_X_ARGS);
    else if (load == kLoadPacked) hipLaunchKernelGGL((rgb_to_x_kernel<kLoadPacked, false>), grid, block, 0, RGB_TO_X_ARGS);
    else if (load == kLoadPlanar && vec_x) hipLaunchKernelGGL((rgb_to_x_kernel<kLoadPlanar, true>), grid, block, 0, RGB_TO_X_ARGS);
    else if (load == kLoadPlanar) hipLaunchKernelGGL((rgb_to_x_kernel<kLoadPlanar, false>), grid, block, 0, RGB_TO_X_ARGS);
    else hipLaunchKernelGGL((rgb_to_x_kernel<kLoadScalar, false>), grid, block, 0, RGB_TO_X_ARGS);
#undef RGB_TO_X_ARGS
    hip_check(hipGetLastError(), "rgb_to_x launch");
}

void x_to_rgb(const half_t* x, int row_pixels, int H, int W, half_t* rgb16, uint8_t* rgb8, hipStream_t stream)
{
    rgb_validate(H, W, "x_to_rgb");
    if (x == nullptr) throw std::invalid_argument("x_to_rgb: no x_hat");
    if (row_pixels < W) throw std::invalid_argument("x_to_rgb: the rows of x_hat are shorter than the picture");
    const bool vec = row_pixels % 8 == 0 && W % 8 == 0 && aligned(x, 16) && (rgb16 == nullptr || aligned(rgb16, 16)) &&
                     (rgb8 == nullptr || aligned(rgb8, 8));
    if (rgb16 == nullptr && rgb8 == nullptr) return;
    const dim3 grid(grid_of(H, W)), block(kThreads);
    if (vec) hipLaunchKernelGGL(x_to_rgb_kernel<true>, grid, block, 0, stream, x, row_pixels, H, W, rgb16, rgb8);
    else hipLaunchKernelGGL(x_to_rgb_kernel<false>, grid, block, 0, stream, x, row_pixels, H, W, rgb16, rgb8);
    hip_check(hipGetLastError(), "x_to_rgb launch");
}

void sse_validate(const SseDesc& d)
{
    if (d.src == nullptr || d.rec == nullptr || d.out == nullptr) throw std::invalid_argument("sse: null operand");
    for (int t : {d.src_dtype, d.rec_dtype}) {
        if (!known_sample(t)) throw std::invalid_argument("sse: unknown sample type " + std::to_string(t));
    }
    if (d.n_planes <= 0 || d.H <= 0 || d.W <= 0) throw std::invalid_argument("sse: empty geometry");
    if (d.n_planes > 65535) throw std::invalid_argument("sse: at most 65535 planes per call");
    // 32-bit piece indices: 8 samples per piece, the last workgroup's stride included
    if (static_cast<long long>(d.H) * ((d.W + 7) / 8) + static_cast<long long>(kSsePartials) * kThreads > (1LL << 31)) {
        throw std::invalid_argument("sse: plane too large");
    }
    if (d.row_stride < d.W) throw std::invalid_argument("sse: row stride below the plane width");
    if (d.n_planes > 1 && d.plane_stride < static_cast<long long>(d.H - 1) * d.row_stride + d.W) {
        throw std::invalid_argument("sse: plane stride below the plane size");
    }
}

size_t sse_workspace_bytes(int n_planes, int H, int W)
{
    return static_cast<size_t>(n_planes) * sse_parts(H, W) * sizeof(double);
}

void sse(const SseDesc& d, void* workspace, hipStream_t stream)
{
    sse_validate(d);
    double* partial = static_cast<double*>(workspace);
    const int parts = sse_parts(d.H, d.W);
    switch (d.src_dtype) {
    case kSampleU8: launch_sse_b(static_cast<const uint8_t*>(d.src), d, partial, parts, stream); break;
    case kSampleF16: launch_sse_b(static_cast<const half_t*>(d.src), d, partial, parts, stream); break;
    case kSampleU16: launch_sse_b(static_cast<const uint16_t*>(d.src), d, partial, parts, stream); break;
    default: launch_sse_b(static_cast<const float*>(d.src), d, partial, parts, stream); break;
    }
    hip_check(hipGetLastError(), "sse launch");
    hipLaunchKernelGGL(sse_final_kernel, dim3(d.n_planes), dim3(kThreads), 0, stream, partial, parts, d.out);
    hip_check(hipGetLastError(), "sse final launch");
}

}  // namespace dcvc
