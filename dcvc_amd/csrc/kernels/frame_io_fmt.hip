// frame_io_fmt.hip - 4:2:0, 4:2:2, 4:4:4 planar and NV12 / P010 pictures of 8..16 bits <-> the codec's fp16 NHWC picture tensor.
//
// One picture is contiguous, in file layout: Y [H][W], then Cb and Cr as planes [2][Hc][Wc] or, for NV12, interleaved
// [Hc][Wc][2]; Hc = H (H / 2 for 4:2:0 and NV12), Wc = W (W / 2 for all but 4:4:4). 8 bits: u8 samples, max_val 255; 9..16
// bits: u16 samples, max_val = 2^b - 1, LSB-aligned in the planar formats and in the high b bits for NV12 (P010 / P012 /
// P016). The arithmetic is frame_io.hip's and frame_io16.hip's, per sample:
//   pix_to_x: d = fp16(fp32(v) / fp32(max_val)) (a correctly rounded division), x = fp16(fp32(d) - 0.5); chroma is
//             nearest-neighbour, sample (h >> sub_h, w >> sub_w); P010 reads v >> (16 - b). `planar` receives the picture as
//             LSB-aligned planar samples at the format's own subsampling (a copy for the planar formats).
//   x_to_pix: t = hadd(x_hat, 0.5); chroma t: the same (4:4:4), fp16((fp32(t_left) + fp32(t_right)) * 0.5f) (4:2:2), or the
//             2 x 2 rule of x_to_yuv420 (fp32 sum in the order (0, 0), (0, 1), (1, 0), (1, 1), fp16(sum * 0.25f)).
//             dist = fp32(scale255(t)) at 8 bits, clamp(fp32(t) * max_val, 0, max_val) at 9..16; samples rint(dist), half to
//             even - but the two 4:2:0 layouts at 8 bits truncate Cb / Cr, as x_to_yuv420 does. P010 stores s << (16 - b).
// So YUV420P and NV12 give the bits of yuv420_to_x / x_to_yuv420 / yuv420p16_to_x / x_to_yuv420p16 up to the layout.
// HBM-bound passes, one thread per 8 luma pixels of a row (8 x 2 for the 4:2:0 writer), 256-thread workgroups, no LDS; 16-B
// accesses where W % 8 == 0, the bases are 16-B aligned and x has ldx == 3 / row_pixels % 8 == 0, element accesses elsewhere.
#include "arith.h"
#include "ops.h"

namespace dcvc {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ half_t load_sample(unsigned v, float maxv)
{
    const half_t d = to_half(static_cast<float>(v) / maxv);        // true division, correctly rounded
    return to_half(static_cast<float>(d) - 0.5f);
}

// frame_io.hip's scale255: the fp16 product and clamp of the 8-bit distortion planes
__device__ __forceinline__ half_t scale255(half_t t)
{
    const float v = static_cast<float>(to_half(static_cast<float>(t) * 255.0f));
    return to_half(fminf(fmaxf(v, 0.f), 255.f));
}

template <int BYTES> struct Raw;
template <> struct Raw<4> { typedef uint32_t type; };
template <> struct Raw<8> { typedef uint2 type; };
template <> struct Raw<16> { typedef uint4 type; };

// N samples behind an N sizeof(T)-aligned address in one access
template <typename T, int N>
__device__ __forceinline__ void load_n(const T* p, unsigned* v)
{
    typedef typename Raw<N * sizeof(T)>::type R;
    const R r = *reinterpret_cast<const R*>(p);
    const T* s = reinterpret_cast<const T*>(&r);
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = s[e];
}

template <typename T, int N>
__device__ __forceinline__ void store_n(T* p, const unsigned* v)
{
    typedef typename Raw<N * sizeof(T)>::type R;
    R r;
    T* s = reinterpret_cast<T*>(&r);
#pragma unroll
    for (int e = 0; e < N; ++e) s[e] = static_cast<T>(v[e]);
    *reinterpret_cast<R*>(p) = r;
}

constexpr bool sub_w(int fmt) { return fmt != kPixYuv444p; }
constexpr bool sub_h(int fmt) { return fmt == kPixYuv420p || fmt == kPixNv12; }

// one thread = 8 consecutive luma pixels of a row and the chroma samples above them. VEC: W % 8 == 0, 16-B aligned bases
// and x at ldx == 3: one access per plane piece, 3 x 16-B stores of x.
template <int FMT, typename T, bool VEC>
__global__ void __launch_bounds__(kThreads) pix_to_x_kernel(const T* __restrict__ src, int H, int W, float maxv, int shift,
                                                            half_t* __restrict__ x, int ldx, T* __restrict__ planar)
{
    constexpr int SW = sub_w(FMT) ? 1 : 0, SH = sub_h(FMT) ? 1 : 0, NC = 8 >> SW;
    const unsigned wv = (W + 7) >> 3;
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;      // < 2^31 (validate)
    if (i >= static_cast<unsigned>(H) * wv) return;
    const int h = static_cast<int>(i / wv), w0 = static_cast<int>(i - h * wv) * 8;
    const int Hc = H >> SH, Wc = W >> SW;
    const size_t plane = static_cast<size_t>(H) * W, cplane = static_cast<size_t>(Hc) * Wc;
    const int n = VEC ? 8 : min(8, W - w0), nc = n >> SW;        // W is even: n is
    const size_t yo = static_cast<size_t>(h) * W + w0;
    const size_t co = static_cast<size_t>(h >> SH) * Wc + (w0 >> SW);      // the thread's first sample in a chroma plane
    unsigned ys[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cb[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (VEC) {
        load_n<T, 8>(src + yo, ys);
        if constexpr (FMT == kPixNv12) {
            unsigned uv[8];
            load_n<T, 8>(src + plane + 2 * co, uv);
#pragma unroll
            for (int k = 0; k < 4; ++k) { cb[k] = uv[2 * k]; cr[k] = uv[2 * k + 1]; }
        } else {
            load_n<T, NC>(src + plane + co, cb);
            load_n<T, NC>(src + plane + cplane + co, cr);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (e < n) ys[e] = src[yo + e];
        }
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            if (k >= nc) continue;
            if constexpr (FMT == kPixNv12) {
                cb[k] = src[plane + 2 * (co + k)];
                cr[k] = src[plane + 2 * (co + k) + 1];
            } else {
                cb[k] = src[plane + co + k];
                cr[k] = src[plane + cplane + co + k];
            }
        }
    }
    if constexpr (FMT == kPixNv12 && sizeof(T) == 2) {         // P010: the value sits in the high bits
#pragma unroll
        for (int e = 0; e < 8; ++e) ys[e] >>= shift;
#pragma unroll
        for (int k = 0; k < NC; ++k) { cb[k] >>= shift; cr[k] >>= shift; }
    }
    if (x) {
        half_t hu[NC], hv[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) { hu[k] = load_sample(cb[k], maxv); hv[k] = load_sample(cr[k], maxv); }
        half_t* o = x + yo * ldx;
        if constexpr (VEC) {
            half8 out[3];
            half_t* ho = reinterpret_cast<half_t*>(out);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                ho[3 * e + 0] = load_sample(ys[e], maxv);
                ho[3 * e + 1] = hu[e >> SW];
                ho[3 * e + 2] = hv[e >> SW];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) reinterpret_cast<half8*>(o)[k] = out[k];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (e >= n) continue;
                o[static_cast<size_t>(e) * ldx + 0] = load_sample(ys[e], maxv);
                o[static_cast<size_t>(e) * ldx + 1] = hu[e >> SW];
                o[static_cast<size_t>(e) * ldx + 2] = hv[e >> SW];
            }
        }
    }
    if (planar) {
        const bool chroma_row = SH == 0 || (h & 1) == 0;       // 4:2:0: the even luma row writes the chroma row
        if constexpr (VEC) {
            store_n<T, 8>(planar + yo, ys);
            if (chroma_row) {
                store_n<T, NC>(planar + plane + co, cb);
                store_n<T, NC>(planar + plane + cplane + co, cr);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (e < n) planar[yo + e] = static_cast<T>(ys[e]);
            }
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                if (k >= nc || !chroma_row) continue;
                planar[plane + co + k] = static_cast<T>(cb[k]);
                planar[plane + cplane + co + k] = static_cast<T>(cr[k]);
            }
        }
    }
}

// fp32 distortion sample of one fp16 t in 0..1
template <bool B8>
__device__ __forceinline__ float dist_of(half_t t, float maxv)
{
    if constexpr (B8) return static_cast<float>(scale255(t));
    else return fminf(fmaxf(static_cast<float>(t) * maxv, 0.f), maxv);
}

// one thread = 8 luma pixels of a row (4:2:2, 4:4:4) or 8 x 2 (4:2:0, NV12) and the chroma samples they average to. VEC:
// W % 8 == 0, row_pixels % 8 == 0 and 16-B aligned bases: 3 x 16-B loads per luma row, one store per output piece.
template <int FMT, typename T, bool VEC>
__global__ void __launch_bounds__(kThreads) x_to_pix_kernel(const half_t* __restrict__ x, int row_pixels, int H, int W, float maxv,
                                                            int shift, float* __restrict__ dist, T* __restrict__ out)
{
    constexpr int SW = sub_w(FMT) ? 1 : 0, SH = sub_h(FMT) ? 1 : 0, NC = 8 >> SW;
    constexpr bool B8 = sizeof(T) == 1;
    constexpr float kMean = SW && SH ? 0.25f : SW ? 0.5f : 1.0f;      // one over the luma pixels of a chroma sample
    const int Hc = H >> SH, Wc = W >> SW;
    const unsigned wv = (W + 7) >> 3;
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;      // < 2^31 (validate)
    if (i >= static_cast<unsigned>(Hc) * wv) return;
    const int hc = static_cast<int>(i / wv), w0 = static_cast<int>(i - hc * wv) * 8;
    const int n = VEC ? 8 : min(8, W - w0), nc = n >> SW;
    const size_t plane = static_cast<size_t>(H) * W, cplane = static_cast<size_t>(Hc) * Wc;
    float su[NC], sv[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) su[k] = sv[k] = 0.f;
    // a chroma sample's luma pixels are summed in the order (0, 0), (0, 1), (1, 0), (1, 1), as x_to_yuv420 does
#pragma unroll
    for (int dy = 0; dy <= SH; ++dy) {
        const int h = (hc << SH) + dy;
        const half_t* p = x + (static_cast<size_t>(h) * row_pixels + w0) * 3;
        half_t px[24];
        if constexpr (VEC) {
#pragma unroll
            for (int k = 0; k < 3; ++k) reinterpret_cast<half8*>(px)[k] = reinterpret_cast<const half8*>(p)[k];
        } else {
#pragma unroll
            for (int e = 0; e < 24; ++e) px[e] = e < 3 * n ? p[e] : static_cast<half_t>(0.f);
        }
        float dy_[8];
        unsigned sy[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            dy_[e] = dist_of<B8>(hadd(px[3 * e], static_cast<half_t>(0.5f)), maxv);           // x_hat + 0.5
            sy[e] = static_cast<unsigned>(rintf(dy_[e])) << shift;                            // half to even
            su[e >> SW] += static_cast<float>(hadd(px[3 * e + 1], static_cast<half_t>(0.5f)));
            sv[e >> SW] += static_cast<float>(hadd(px[3 * e + 2], static_cast<half_t>(0.5f)));
        }
        const size_t o = static_cast<size_t>(h) * W + w0;
        if constexpr (VEC) {
            if (dist) {
                reinterpret_cast<float4*>(dist + o)[0] = make_float4(dy_[0], dy_[1], dy_[2], dy_[3]);
                reinterpret_cast<float4*>(dist + o)[1] = make_float4(dy_[4], dy_[5], dy_[6], dy_[7]);
            }
            if (out) store_n<T, 8>(out + o, sy);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (e >= n) continue;
                if (dist) dist[o + e] = dy_[e];
                if (out) out[o + e] = static_cast<T>(sy[e]);
            }
        }
    }
    // avg_pool2d accumulates in fp32 and rounds once (4:4:4: fp16(fp32(t) * 1) is t)
    float du[NC], dv[NC];
    unsigned cu[NC], cv[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        du[k] = dist_of<B8>(to_half(su[k] * kMean), maxv);
        dv[k] = dist_of<B8>(to_half(sv[k] * kMean), maxv);
        if constexpr (B8 && SH) {                               // the reference writer's .byte(): truncation
            cu[k] = static_cast<unsigned>(du[k]);
            cv[k] = static_cast<unsigned>(dv[k]);
        } else {
            cu[k] = static_cast<unsigned>(rintf(du[k])) << shift;
            cv[k] = static_cast<unsigned>(rintf(dv[k])) << shift;
        }
    }
    const size_t co = static_cast<size_t>(hc) * Wc + (w0 >> SW);
    if constexpr (VEC) {
        if (dist) {
#pragma unroll
            for (int k = 0; k < NC; k += 4) {
                *reinterpret_cast<float4*>(dist + plane + co + k) = make_float4(du[k], du[k + 1], du[k + 2], du[k + 3]);
                *reinterpret_cast<float4*>(dist + plane + cplane + co + k) = make_float4(dv[k], dv[k + 1], dv[k + 2], dv[k + 3]);
            }
        }
        if (out) {
            if constexpr (FMT == kPixNv12) {
                unsigned uv[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) { uv[2 * k] = cu[k]; uv[2 * k + 1] = cv[k]; }
                store_n<T, 8>(out + plane + 2 * co, uv);
            } else {
                store_n<T, NC>(out + plane + co, cu);
                store_n<T, NC>(out + plane + cplane + co, cv);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            if (k >= nc) continue;
            if (dist) { dist[plane + co + k] = du[k]; dist[plane + cplane + co + k] = dv[k]; }
            if (out) {
                if constexpr (FMT == kPixNv12) {
                    out[plane + 2 * (co + k)] = static_cast<T>(cu[k]);
                    out[plane + 2 * (co + k) + 1] = static_cast<T>(cv[k]);
                } else {
                    out[plane + co + k] = static_cast<T>(cu[k]);
                    out[plane + cplane + co + k] = static_cast<T>(cv[k]);
                }
            }
        }
    }
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

void validate(int fmt, int bit_depth, int H, int W, const char* what)
{
    if (fmt < kPixYuv420p || fmt > kPixNv12) {
        throw std::invalid_argument(std::string(what) + ": unknown pixel format " + std::to_string(fmt));
    }
    if (bit_depth < 8 || bit_depth > 16) {
        throw std::invalid_argument(std::string(what) + ": bit depth must be 8..16, got " + std::to_string(bit_depth));
    }
    if (H <= 0 || W <= 0 || (H & 1) || (W & 1)) {
        throw std::invalid_argument(std::string(what) + ": the picture sides must be positive and even, got " +
                                    std::to_string(W) + "x" + std::to_string(H));
    }
    // one thread per 8 pixels of a row, 32-bit thread indices (addresses are 64-bit)
    if (static_cast<long long>(H) * ((W + 7) / 8) + kThreads > (1LL << 31)) throw std::invalid_argument(std::string(what) + ": picture too large");
}

float max_val(int bit_depth) { return static_cast<float>((1 << bit_depth) - 1); }      // exact in fp32 up to 16 bits

// P010 and its relatives keep the value in the high bits of the u16
int msb_shift(int fmt, int bit_depth) { return fmt == kPixNv12 && bit_depth > 8 ? 16 - bit_depth : 0; }

dim3 grid_of(long long threads) { return dim3(static_cast<unsigned>((threads + kThreads - 1) / kThreads)); }

template <int FMT, typename T>
void launch_to_x(bool vec, long long n, hipStream_t stream, const void* src, int H, int W, float maxv, int shift, half_t* x, int ldx,
                 void* planar)
{
    if (vec) hipLaunchKernelGGL((pix_to_x_kernel<FMT, T, true>), grid_of(n), dim3(kThreads), 0, stream, static_cast<const T*>(src), H, W,
                                maxv, shift, x, ldx, static_cast<T*>(planar));
    else hipLaunchKernelGGL((pix_to_x_kernel<FMT, T, false>), grid_of(n), dim3(kThreads), 0, stream, static_cast<const T*>(src), H, W,
                            maxv, shift, x, ldx, static_cast<T*>(planar));
}

template <int FMT, typename T>
void launch_to_pix(bool vec, long long n, hipStream_t stream, const half_t* x, int row_pixels, int H, int W, float maxv, int shift,
                   float* dist, void* out)
{
    if (vec) hipLaunchKernelGGL((x_to_pix_kernel<FMT, T, true>), grid_of(n), dim3(kThreads), 0, stream, x, row_pixels, H, W, maxv, shift,
                                dist, static_cast<T*>(out));
    else hipLaunchKernelGGL((x_to_pix_kernel<FMT, T, false>), grid_of(n), dim3(kThreads), 0, stream, x, row_pixels, H, W, maxv, shift,
                            dist, static_cast<T*>(out));
}

}  // namespace

long long pix_picture_samples(int fmt, int H, int W)
{
    validate(fmt, 8, H, W, "pix_picture_samples");
    const long long hc = sub_h(fmt) ? H / 2 : H, wc = sub_w(fmt) ? W / 2 : W;
    return static_cast<long long>(H) * W + 2 * hc * wc;
}

void pix_to_x(const void* src, int fmt, int bit_depth, int H, int W, half_t* x, int ldx, void* planar, hipStream_t stream)
{
    validate(fmt, bit_depth, H, W, "pix_to_x");
    if (src == nullptr) throw std::invalid_argument("pix_to_x: null source");
    if (x == nullptr && planar == nullptr) throw std::invalid_argument("pix_to_x: x and planar are both null");
    if (x != nullptr && ldx < 3) throw std::invalid_argument("pix_to_x: the pixel stride of x must be >= 3");
    // W % 8 == 0 keeps every row and every plane of the picture on the boundary of its access behind a 16-B aligned base:
    // H W, Hc Wc and Wc are multiples of 4 samples (of 8 where 8 are accessed at once)
    const bool vec = W % 8 == 0 && aligned(src, 16) && (x == nullptr || (ldx == 3 && aligned(x, 16))) &&
                     (planar == nullptr || aligned(planar, 16));
    const long long n = static_cast<long long>(H) * ((W + 7) / 8);
    const float maxv = max_val(bit_depth);
    const int shift = msb_shift(fmt, bit_depth);
#define DCVC_PIX_TO_X(F)                                                                                          \
    case F:                                                                                                       \
        if (bit_depth == 8) launch_to_x<F, uint8_t>(vec, n, stream, src, H, W, maxv, shift, x, ldx, planar);       \
        else launch_to_x<F, uint16_t>(vec, n, stream, src, H, W, maxv, shift, x, ldx, planar);                     \
        break;
    switch (fmt) {
        DCVC_PIX_TO_X(kPixYuv420p)
        DCVC_PIX_TO_X(kPixYuv422p)
        DCVC_PIX_TO_X(kPixYuv444p)
        DCVC_PIX_TO_X(kPixNv12)
    }
#undef DCVC_PIX_TO_X
    hip_check(hipGetLastError(), "pix_to_x launch");
}

void x_to_pix(const half_t* x, int row_pixels, int H, int W, int fmt, int bit_depth, float* dist, void* out, hipStream_t stream)
{
    validate(fmt, bit_depth, H, W, "x_to_pix");
    if (x == nullptr) throw std::invalid_argument("x_to_pix: no x_hat");
    if (row_pixels < W) throw std::invalid_argument("x_to_pix: the rows of x_hat are shorter than the picture");
    if (dist == nullptr && out == nullptr) return;
    const bool vec = W % 8 == 0 && row_pixels % 8 == 0 && aligned(x, 16) && (dist == nullptr || aligned(dist, 16)) &&
                     (out == nullptr || aligned(out, 16));
    const long long n = static_cast<long long>(sub_h(fmt) ? H / 2 : H) * ((W + 7) / 8);
    const float maxv = max_val(bit_depth);
    const int shift = msb_shift(fmt, bit_depth);
#define DCVC_X_TO_PIX(F)                                                                                          \
    case F:                                                                                                       \
        if (bit_depth == 8) launch_to_pix<F, uint8_t>(vec, n, stream, x, row_pixels, H, W, maxv, shift, dist, out);   \
        else launch_to_pix<F, uint16_t>(vec, n, stream, x, row_pixels, H, W, maxv, shift, dist, out);                 \
        break;
    switch (fmt) {
        DCVC_X_TO_PIX(kPixYuv420p)
        DCVC_X_TO_PIX(kPixYuv422p)
        DCVC_X_TO_PIX(kPixYuv444p)
        DCVC_X_TO_PIX(kPixNv12)
    }
#undef DCVC_X_TO_PIX
    hip_check(hipGetLastError(), "x_to_pix launch");
}

}  // namespace dcvc
