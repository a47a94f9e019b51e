// picture_yuv.hip - YUV pictures of 8..16 bits (4:2:0, 4:2:2, 4:4:4 planar and NV12 / P010) <-> the codec's fp16 NHWC picture
// tensor: one kernel to x and one from x behind pix_to_x / x_to_pix and the older 4:2:0 entries yuv420_to_x / x_to_yuv420
// (8 bits) and yuv420p16_to_x / x_to_yuv420p16 (9..16 bits), which hand over their planes where the former take one picture.
//
// A picture is Y [H][W] behind the luma base and, behind the chroma base, Cb and Cr as planes [2][Hc][Wc] or, for NV12,
// interleaved [Hc][Wc][2]; Hc = H (H / 2 for 4:2:0 and NV12), Wc = W (W / 2 for all but 4:4:4). In file layout the chroma base
// is the luma base + H W. 8 bits: u8 samples, max_val 255; 9..16 bits: u16 samples, max_val = 2^b - 1, LSB-aligned in the
// planar formats and in the high b bits for NV12 (P010 / P012 / P016).
// Reference: test_video.py:69-123 get_src_frame (nearest-neighbour chroma, .half(), / 255, - 0.5), :32-45 get_distortion and
// :356-363 (x_hat + 0.5, 2 x 2 average of the chroma, * 255, clamp; the writer rounds Y half to even and TRUNCATES U / V);
// DCVC-FM's YUVReader / YUVWriter (video_reader.py:130-183, video_writer.py:86-130) for the scale of 9..16-bit samples.
//   to x:   d = fp16(fp32(v) / fp32(max_val)) (a correctly rounded division: the library builds with -fno-fast-math),
//           x = fp16(fp32(d) - 0.5); chroma is nearest-neighbour, sample (h >> sub_h, w >> sub_w); P010 reads v >> (16 - b).
//           Samples above max_val are neither masked nor checked. `planar` receives the picture as LSB-aligned planar samples
//           at the format's own subsampling (a copy for the planar formats).
//   from x: t = hadd(x_hat, 0.5); chroma t: the same (4:4:4), fp16((fp32(t_left) + fp32(t_right)) * 0.5f) (4:2:2), or the
//           2 x 2 rule (fp32 sum in the order (0, 0), (0, 1), (1, 0), (1, 1), fp16(sum * 0.25f): avg_pool2d).
//           dist = fp32(scale255(t)) at 8 bits, clamp(fp32(t) * max_val, 0, max_val) at 9..16 (fp16 cannot hold a 10-bit
//           sample to better than 0.5); samples rint(dist), half to even - but the two 4:2:0 layouts at 8 bits truncate
//           Cb / Cr, as the reference's writer does. P010 stores s << (16 - b). x_to_yuv420 stores dist as fp16, which at
//           8 bits holds the same values.
// HBM-bound passes, one thread per 8 luma pixels of a row (8 x 2 for the 4:2:0 writer), 256-thread workgroups, no LDS. Where
// W % 8 == 0, x has ldx == 3 / row_pixels % 8 == 0 and every base is aligned for the piece a thread accesses behind it (16 B,
// or the piece's size where that is less: 8 u8 luma samples, 4 chroma samples), one access per piece; element accesses
// elsewhere (chunk slots at ldx = 24, widths that are no multiple of 8, planes at odd addresses).
#include "arith.h"
#include "picture_io.h"

namespace dcvc {

namespace {

constexpr int kThreads = kPictureThreads;

__device__ __forceinline__ half_t load_sample(unsigned v, float maxv)
{
    const half_t d = to_half(static_cast<float>(v) / maxv);        // true division, correctly rounded
    return to_half(static_cast<float>(d) - 0.5f);
}

// the fp16 product and clamp of the 8-bit distortion planes
__device__ __forceinline__ half_t scale255(half_t t)
{
    const float v = static_cast<float>(to_half(static_cast<float>(t) * 255.0f));
    return to_half(fminf(fmaxf(v, 0.f), 255.f));
}

template <int BYTES> struct Raw;
template <> struct Raw<4> { typedef uint32_t type; };
template <> struct Raw<8> { typedef uint2 type; };
template <> struct Raw<16> { typedef uint4 type; };

// the bytes of one access to N samples of T: 16, or all of them where that is less
template <typename T, int N> constexpr int piece_bytes() { return N * sizeof(T) < 16 ? static_cast<int>(N * sizeof(T)) : 16; }

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

// N distortion samples (fp32, or fp16 of the same value) behind a piece_bytes-aligned address in accesses of that size
template <typename D, int N>
__device__ __forceinline__ void store_dist(D* p, const float* v)
{
    typedef typename Raw<piece_bytes<D, N>()>::type R;
    constexpr int K = N * sizeof(D) / sizeof(R);
    R r[K];
    D* s = reinterpret_cast<D*>(r);
#pragma unroll
    for (int e = 0; e < N; ++e) s[e] = static_cast<D>(v[e]);
#pragma unroll
    for (int k = 0; k < K; ++k) reinterpret_cast<R*>(p)[k] = r[k];
}

constexpr bool sub_w(int fmt) { return fmt != kPixYuv444p; }
constexpr bool sub_h(int fmt) { return fmt == kPixYuv420p || fmt == kPixNv12; }
// the chroma samples a thread accesses at once behind the chroma base: its 8 >> sub_w Cb (and as many Cr), NV12: the 8 of both
constexpr int chroma_piece(int fmt) { return fmt == kPixYuv444p || fmt == kPixNv12 ? 8 : 4; }

// one thread = 8 consecutive luma pixels of a row and the chroma samples above them; yp, cp: the luma and the chroma base.
// VEC (host: to_x_vec): one access per plane piece, 3 x 16-B stores of x.
template <int FMT, typename T, bool VEC>
__global__ void __launch_bounds__(kThreads) pix_to_x_kernel(const T* __restrict__ yp, const T* __restrict__ cp, int H, int W,
                                                            float maxv, int shift, half_t* __restrict__ x, int ldx,
                                                            T* __restrict__ planar)
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
        load_n<T, 8>(yp + yo, ys);
        if constexpr (FMT == kPixNv12) {
            unsigned uv[8];
            load_n<T, 8>(cp + 2 * co, uv);
#pragma unroll
            for (int k = 0; k < 4; ++k) { cb[k] = uv[2 * k]; cr[k] = uv[2 * k + 1]; }
        } else {
            load_n<T, NC>(cp + co, cb);
            load_n<T, NC>(cp + cplane + co, cr);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (e < n) ys[e] = yp[yo + e];
        }
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            if (k >= nc) continue;
            if constexpr (FMT == kPixNv12) {
                cb[k] = cp[2 * (co + k)];
                cr[k] = cp[2 * (co + k) + 1];
            } else {
                cb[k] = cp[co + k];
                cr[k] = cp[cplane + co + k];
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

// one thread = 8 luma pixels of a row (4:2:2, 4:4:4) or 8 x 2 (4:2:0, NV12) and the chroma samples they average to. dist_y,
// dist_c: the luma and the chroma base of the distortion planes (D: fp32, or fp16 of the same value), out_y, out_c: of the
// samples; each may be null. VEC (host: from_x_vec): 3 x 16-B loads per luma row, one or two stores per output piece.
template <int FMT, typename T, typename D, bool VEC>
__global__ void __launch_bounds__(kThreads) x_to_pix_kernel(const half_t* __restrict__ x, int row_pixels, int H, int W, float maxv,
                                                            int shift, D* __restrict__ dist_y, D* __restrict__ dist_c,
                                                            T* __restrict__ out_y, T* __restrict__ out_c)
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
    const size_t cplane = static_cast<size_t>(Hc) * Wc;
    float su[NC], sv[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) su[k] = sv[k] = 0.f;
    // a chroma sample's luma pixels are summed in the order (0, 0), (0, 1), (1, 0), (1, 1), as avg_pool2d does
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
            if (dist_y) store_dist<D, 8>(dist_y + o, dy_);
            if (out_y) store_n<T, 8>(out_y + o, sy);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (e >= n) continue;
                if (dist_y) dist_y[o + e] = static_cast<D>(dy_[e]);
                if (out_y) out_y[o + e] = static_cast<T>(sy[e]);
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
        if (dist_c) {
            store_dist<D, NC>(dist_c + co, du);
            store_dist<D, NC>(dist_c + cplane + co, dv);
        }
        if (out_c) {
            if constexpr (FMT == kPixNv12) {
                unsigned uv[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) { uv[2 * k] = cu[k]; uv[2 * k + 1] = cv[k]; }
                store_n<T, 8>(out_c + 2 * co, uv);
            } else {
                store_n<T, NC>(out_c + co, cu);
                store_n<T, NC>(out_c + cplane + co, cv);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            if (k >= nc) continue;
            if (dist_c) { dist_c[co + k] = static_cast<D>(du[k]); dist_c[cplane + co + k] = static_cast<D>(dv[k]); }
            if (out_c) {
                if constexpr (FMT == kPixNv12) {
                    out_c[2 * (co + k)] = static_cast<T>(cu[k]);
                    out_c[2 * (co + k) + 1] = static_cast<T>(cv[k]);
                } else {
                    out_c[co + k] = static_cast<T>(cu[k]);
                    out_c[cplane + co + k] = static_cast<T>(cv[k]);
                }
            }
        }
    }
}

// min_depth: 8, or 9 for the entries that take u16 samples only
void validate(int fmt, int bit_depth, int min_depth, int H, int W, const char* what)
{
    if (fmt < kPixYuv420p || fmt > kPixNv12) {
        throw std::invalid_argument(std::string(what) + ": unknown pixel format " + std::to_string(fmt));
    }
    if (bit_depth < min_depth || bit_depth > 16) {
        throw std::invalid_argument(std::string(what) + ": bit depth must be " + std::to_string(min_depth) + "..16, got " +
                                    std::to_string(bit_depth));
    }
    picture_validate(H, W, what);
}

float max_val(int bit_depth) { return static_cast<float>((1 << bit_depth) - 1); }      // exact in fp32 up to 16 bits

// P010 and its relatives keep the value in the high bits of the u16
int msb_shift(int fmt, int bit_depth) { return fmt == kPixNv12 && bit_depth > 8 ? 16 - bit_depth : 0; }

// a null base is not accessed
bool aligned_or_null(const void* p, size_t a) { return p == nullptr || aligned(p, a); }

// what every entry to x hands over once its own operands are checked: the picture behind its two bases
struct ToX {
    int fmt, bit_depth, H, W;
    const void* y; const void* c;
    half_t* x; int ldx;
    void* planar;
};

// W % 8 == 0 keeps every row and every plane behind a base on the boundary of its access when the base is: H W, Hc Wc and Wc
// are multiples of 4 samples (of 8 where 8 are accessed at once)
template <int FMT, typename T>
void launch_to_x(const ToX& a, hipStream_t stream)
{
    const bool vec = a.W % 8 == 0 && aligned(a.y, piece_bytes<T, 8>()) && aligned(a.c, piece_bytes<T, chroma_piece(FMT)>()) &&
                     (a.x == nullptr || (a.ldx == 3 && aligned(a.x, 16))) && aligned_or_null(a.planar, 16);
    const dim3 grid(grid_of(a.H, a.W)), block(kThreads);
    const float maxv = max_val(a.bit_depth);
    const int shift = msb_shift(FMT, a.bit_depth);
    const T* y = static_cast<const T*>(a.y);
    const T* c = static_cast<const T*>(a.c);
    T* planar = static_cast<T*>(a.planar);
    if (vec) hipLaunchKernelGGL((pix_to_x_kernel<FMT, T, true>), grid, block, 0, stream, y, c, a.H, a.W, maxv, shift, a.x, a.ldx, planar);
    else hipLaunchKernelGGL((pix_to_x_kernel<FMT, T, false>), grid, block, 0, stream, y, c, a.H, a.W, maxv, shift, a.x, a.ldx, planar);
}

void to_x(const ToX& a, const char* what, hipStream_t stream)
{
    if (a.x != nullptr && a.ldx < 3) throw std::invalid_argument(std::string(what) + ": the pixel stride of x must be >= 3");
#define DCVC_PIX_TO_X(F)                                              \
    case F:                                                           \
        if (a.bit_depth == 8) launch_to_x<F, uint8_t>(a, stream);     \
        else launch_to_x<F, uint16_t>(a, stream);                     \
        break;
    switch (a.fmt) {
        DCVC_PIX_TO_X(kPixYuv420p)
        DCVC_PIX_TO_X(kPixYuv422p)
        DCVC_PIX_TO_X(kPixYuv444p)
        DCVC_PIX_TO_X(kPixNv12)
    }
#undef DCVC_PIX_TO_X
    hip_check(hipGetLastError(), (std::string(what) + " launch").c_str());
}

// what every entry from x hands over: x_hat and the four bases, each of which may be null
template <typename D>
struct FromX {
    int fmt, bit_depth;
    const half_t* x; int row_pixels, H, W;
    D* dist_y; D* dist_c;
    void* out_y; void* out_c;
};

// false: nothing to write
template <typename D>
bool from_x_checked(const FromX<D>& a, const char* what)
{
    if (a.x == nullptr) throw std::invalid_argument(std::string(what) + ": no x_hat");
    if (a.row_pixels < a.W) throw std::invalid_argument(std::string(what) + ": the rows of x_hat are shorter than the picture");
    return a.dist_y != nullptr || a.dist_c != nullptr || a.out_y != nullptr || a.out_c != nullptr;
}

template <int FMT, typename T, typename D>
void launch_from_x(const FromX<D>& a, hipStream_t stream)
{
    constexpr int NC = sub_w(FMT) ? 4 : 8;
    const bool vec = a.W % 8 == 0 && a.row_pixels % 8 == 0 && aligned(a.x, 16) && aligned_or_null(a.dist_y, piece_bytes<D, 8>()) &&
                     aligned_or_null(a.dist_c, piece_bytes<D, NC>()) && aligned_or_null(a.out_y, piece_bytes<T, 8>()) &&
                     aligned_or_null(a.out_c, piece_bytes<T, chroma_piece(FMT)>());
    const dim3 grid(grid_of(sub_h(FMT) ? a.H / 2 : a.H, a.W)), block(kThreads);
    const float maxv = max_val(a.bit_depth);
    const int shift = msb_shift(FMT, a.bit_depth);
    T* oy = static_cast<T*>(a.out_y);
    T* oc = static_cast<T*>(a.out_c);
    if (vec) hipLaunchKernelGGL((x_to_pix_kernel<FMT, T, D, true>), grid, block, 0, stream, a.x, a.row_pixels, a.H, a.W, maxv, shift,
                                a.dist_y, a.dist_c, oy, oc);
    else hipLaunchKernelGGL((x_to_pix_kernel<FMT, T, D, false>), grid, block, 0, stream, a.x, a.row_pixels, a.H, a.W, maxv, shift,
                            a.dist_y, a.dist_c, oy, oc);
}

void from_x(const FromX<float>& a, const char* what, hipStream_t stream)
{
    if (!from_x_checked(a, what)) return;
#define DCVC_X_TO_PIX(F)                                                        \
    case F:                                                                     \
        if (a.bit_depth == 8) launch_from_x<F, uint8_t, float>(a, stream);      \
        else launch_from_x<F, uint16_t, float>(a, stream);                      \
        break;
    switch (a.fmt) {
        DCVC_X_TO_PIX(kPixYuv420p)
        DCVC_X_TO_PIX(kPixYuv422p)
        DCVC_X_TO_PIX(kPixYuv444p)
        DCVC_X_TO_PIX(kPixNv12)
    }
#undef DCVC_X_TO_PIX
    hip_check(hipGetLastError(), (std::string(what) + " launch").c_str());
}

}  // namespace

long long pix_picture_samples(int fmt, int H, int W)
{
    validate(fmt, 8, 8, H, W, "pix_picture_samples");
    const long long hc = sub_h(fmt) ? H / 2 : H, wc = sub_w(fmt) ? W / 2 : W;
    return static_cast<long long>(H) * W + 2 * hc * wc;
}

void pix_to_x(const void* src, int fmt, int bit_depth, int H, int W, half_t* x, int ldx, void* planar, hipStream_t stream)
{
    validate(fmt, bit_depth, 8, H, W, "pix_to_x");
    if (src == nullptr) throw std::invalid_argument("pix_to_x: null source");
    if (x == nullptr && planar == nullptr) throw std::invalid_argument("pix_to_x: x and planar are both null");
    const size_t plane = static_cast<size_t>(H) * W * (bit_depth == 8 ? 1 : 2);
    to_x({fmt, bit_depth, H, W, src, static_cast<const char*>(src) + plane, x, ldx, planar}, "pix_to_x", stream);
}

void x_to_pix(const half_t* x, int row_pixels, int H, int W, int fmt, int bit_depth, float* dist, void* out, hipStream_t stream)
{
    validate(fmt, bit_depth, 8, H, W, "x_to_pix");
    const size_t plane = static_cast<size_t>(H) * W;
    from_x({fmt, bit_depth, x, row_pixels, H, W, dist, dist ? dist + plane : nullptr, out,
            out ? static_cast<char*>(out) + plane * (bit_depth == 8 ? 1 : 2) : nullptr}, "x_to_pix", stream);
}

void yuv420_to_x(const uint8_t* y, const uint8_t* uv, int H, int W, half_t* x, int ldx, hipStream_t stream)
{
    validate(kPixYuv420p, 8, 8, H, W, "yuv420_to_x");
    if (y == nullptr || uv == nullptr || x == nullptr) throw std::invalid_argument("yuv420_to_x: null operand");
    to_x({kPixYuv420p, 8, H, W, y, uv, x, ldx, nullptr}, "yuv420_to_x", stream);
}

void x_to_yuv420(const half_t* x, int row_pixels, int H, int W, half_t* y16, half_t* uv16, uint8_t* y8, uint8_t* uv8, hipStream_t stream)
{
    validate(kPixYuv420p, 8, 8, H, W, "x_to_yuv420");
    const FromX<half_t> a = {kPixYuv420p, 8, x, row_pixels, H, W, y16, uv16, y8, uv8};
    if (!from_x_checked(a, "x_to_yuv420")) return;
    launch_from_x<kPixYuv420p, uint8_t, half_t>(a, stream);
    hip_check(hipGetLastError(), "x_to_yuv420 launch");
}

void yuv420p16_to_x(const uint16_t* y, const uint16_t* uv, int H, int W, int bit_depth, half_t* x, int ldx, hipStream_t stream)
{
    validate(kPixYuv420p, bit_depth, 9, H, W, "yuv420p16_to_x");
    if (y == nullptr || uv == nullptr || x == nullptr) throw std::invalid_argument("yuv420p16_to_x: null operand");
    to_x({kPixYuv420p, bit_depth, H, W, y, uv, x, ldx, nullptr}, "yuv420p16_to_x", stream);
}

void x_to_yuv420p16(const half_t* x, int row_pixels, int H, int W, int bit_depth, float* dist, uint16_t* yuv, hipStream_t stream)
{
    validate(kPixYuv420p, bit_depth, 9, H, W, "x_to_yuv420p16");
    const size_t plane = static_cast<size_t>(H) * W;
    from_x({kPixYuv420p, bit_depth, x, row_pixels, H, W, dist, dist ? dist + plane : nullptr, yuv, yuv ? yuv + plane : nullptr},
           "x_to_yuv420p16", stream);
}

}  // namespace dcvc
