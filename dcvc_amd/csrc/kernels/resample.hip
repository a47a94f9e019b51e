// resample.hip - planes of integer samples at another size: a separable Lanczos-3 filter with 12-bit integer
// coefficients, so that every output sample is defined exactly and a numpy restatement can be held against it with ==.
//
// One 1-D pass n_in -> n_out, tables built on the host in IEEE double (no fast-math, no contraction: the library's flags):
//   scale = n_in / n_out, fs = max(1, scale), support = 3 fs, T = 2 ceil(support) taps for every output;
//   output j: centre = (j + 0.5) scale - 0.5, first = floor(centre - support) + 1,
//   w[k] = L((first + k - centre) / fs), L(t) = sinc(t) sinc(t / 3) for |t| < 3, else 0,
//   c[k] = rint(w[k] * 4096 / sum w), and 4096 - sum c is added to the largest c (the first one on a tie): a row sums to 4096.
//   out[j] = clamp((sum_k c[k] in[clamp(first + k, 0, n_in - 1)] + 2048) >> 12, 0, max_val), the shift arithmetic.
// A plane is resampled horizontally into an intermediate plane of clamped samples [in_h][out_w], then vertically.
//
// The accumulator is a signed 32-bit integer. A row's sum |c| is at most kMaxAbsCoefSum (resample_taps refuses a table above it;
// the largest seen over 2:1, 1:2, 3:2, 2:3, 4:1, 1920 -> 854 and 427 -> 960 is 6324), so with 16-bit samples
// |sum| + 2048 <= 32767 * 65535 + 2048 < 2^31.
//
// Horizontal pass: a workgroup of 256 threads makes a tile of kHTile outputs x kHRows rows. The tile's coefficients go to LDS
// transposed ([tap][output]: a thread reads the taps of its 4 outputs as one 8-byte word), the rows' input segment with its
// halo goes to LDS with the edge clamp applied while it is staged - at most T + 16 + kHTile * scale samples a row, the plan
// holds the exact figure - in 16-byte loads where the source allows (VEC_IN), sample by sample otherwise. A thread makes 4
// consecutive outputs of a row and stores them as one word into the intermediate plane, whose pitch is a multiple of 16.
// Vertical pass: threads along x, 8 samples each (8- or 16-byte loads, coalesced as they are), each thread walks its T rows
// with the row index clamped; the row's coefficients are wave-uniform. One 8- or 16-byte store where dst allows (VEC_OUT).
// Planes of one size ride in blockIdx.z: two launches a call, whatever n_planes is. Plane offsets are 64-bit.
#include "ops.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace dcvc {

namespace {

constexpr int kThreads = 256;
constexpr int kHTile = 128;                  // outputs of a horizontal tile: 32 threads x 4
constexpr int kHRows = 16;                   // rows of a horizontal tile: 8 threads x 2
constexpr int kAlign = 16;                   // samples: staged segments start on a multiple of it, pitches are multiples of it
constexpr int kVSamples = 8;                 // samples of a vertical-pass thread
constexpr int kVRows = kThreads / 64;        // output rows of a vertical-pass workgroup
constexpr int kMaxAbsCoefSum = 32767;
static_assert(static_cast<long long>(kMaxAbsCoefSum) * 65535 + 2048 < (1LL << 31), "the 32-bit accumulator must hold a row");
static_assert(kResampleMaxTaps == 2 * 3 * kResampleMaxRatio, "T = 2 ceil(3 max(1, scale))");
// the horizontal tile in LDS at the widest ratio, 16-bit samples: coefficients + rows
constexpr int kMaxHSpan = kHTile * kResampleMaxRatio + kResampleMaxTaps + 2 * kAlign;
static_assert(kResampleMaxTaps * kHTile * 2 + kHRows * kMaxHSpan * 2 <= 64 * 1024, "the horizontal tile must fit the LDS");

double lanczos3(double t)
{
    if (!(std::fabs(t) < 3.0)) return 0.0;
    if (t == 0.0) return 1.0;
    const double a = M_PI * t;
    const double u = t / 3.0;
    const double b = M_PI * u;
    return (std::sin(a) / a) * (std::sin(b) / b);
}

template <typename T> struct Vec16;                                     // a 16-byte vector's worth of samples
template <> struct Vec16<uint8_t> { static constexpr int n = 16; };
template <> struct Vec16<uint16_t> { static constexpr int n = 8; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int finish(int acc, int max_val) { return clampi((acc + 2048) >> 12, 0, max_val); }

template <typename T, bool VEC_IN>
__global__ void __launch_bounds__(kThreads)
resample_h_kernel(const T* __restrict__ src, long long row_stride, long long plane_stride, int in_h, int in_w, T* __restrict__ mid,
                  int pitch, int out_w, const int16_t* __restrict__ coef, const int32_t* __restrict__ first, int taps, int span,
                  int max_val)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    int16_t* cs = reinterpret_cast<int16_t*>(lds);                                     // [taps][kHTile]
    T* ss = reinterpret_cast<T*>(lds + static_cast<size_t>(taps) * kHTile * 2);        // [kHRows][span]
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * kHTile, nj = min(kHTile, out_w - j0);
    const int r0 = blockIdx.y * kHRows, nr = min(kHRows, in_h - r0);
    const long long plane = blockIdx.z;
    // the segment starts at a multiple of kAlign at or below the first tap of the tile's first output (floor: first may be
    // negative); `first` does not decrease with j, and the plan has checked that every tile ends inside `span`
    const int f0 = first[j0];
    const int base = (f0 >= 0 ? f0 / kAlign : -((-f0 + kAlign - 1) / kAlign)) * kAlign;
    for (int i = tid; i < taps * kHTile; i += kThreads) {
        const int o = i / taps, k = i - o * taps;
        cs[k * kHTile + o] = o < nj ? coef[static_cast<long long>(j0) * taps + i] : static_cast<int16_t>(0);
    }
    constexpr int V = Vec16<T>::n;
    const int chunks = span / V;
    const T* splane = src + plane * plane_stride;
    for (int i = tid; i < nr * chunks; i += kThreads) {
        const int r = i / chunks, c = i - r * chunks;
        const int g = base + c * V;
        const T* row = splane + static_cast<long long>(r0 + r) * row_stride;
        T* d = ss + r * span + c * V;
        if (VEC_IN && g >= 0 && g + V <= in_w) {
            *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(row + g);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) d[e] = row[clampi(g + e, 0, in_w - 1)];
        }
    }
    __syncthreads();
    const int o = (tid & 31) * 4;
    if (o >= nj) return;
    int off[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) off[e] = first[min(j0 + o + e, out_w - 1)] - base;      // outputs past out_w: zero coefficients
    for (int r = tid >> 5; r < nr; r += kThreads / 32) {
        const T* s = ss + r * span;
        int acc[4] = {0, 0, 0, 0};
        for (int k = 0; k < taps; ++k) {
            const short4 c = *reinterpret_cast<const short4*>(cs + k * kHTile + o);
            acc[0] += static_cast<int>(c.x) * static_cast<int>(s[off[0] + k]);
            acc[1] += static_cast<int>(c.y) * static_cast<int>(s[off[1] + k]);
            acc[2] += static_cast<int>(c.z) * static_cast<int>(s[off[2] + k]);
            acc[3] += static_cast<int>(c.w) * static_cast<int>(s[off[3] + k]);
        }
        unsigned v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = static_cast<unsigned>(finish(acc[e], max_val));
        T* d = mid + (plane * in_h + (r0 + r)) * pitch + j0 + o;
        if (o + 4 <= nj) {
            if constexpr (sizeof(T) == 1) {
                *reinterpret_cast<unsigned*>(d) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
            } else {
                *reinterpret_cast<uint2*>(d) = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
            }
        } else {
            for (int e = 0; e < nj - o; ++e) d[e] = static_cast<T>(v[e]);
        }
    }
}

template <typename T, bool VEC_OUT>
__global__ void __launch_bounds__(kThreads)
resample_v_kernel(const T* __restrict__ mid, int pitch, int in_h, T* __restrict__ dst, long long row_stride, long long plane_stride,
                  int out_h, int out_w, const int16_t* __restrict__ coef, const int32_t* __restrict__ first, int taps, int max_val)
{
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * kVSamples;
    const int i = blockIdx.y * kVRows + (threadIdx.x >> 6);                      // one output row per wave
    const long long plane = blockIdx.z;
    if (x0 >= out_w || i >= out_h) return;
    const int16_t* c = coef + static_cast<long long>(i) * taps;
    const int f = first[i];
    // the last thread of a row may read past out_w: inside the pitch (a multiple of kAlign), and what it makes of it is not stored
    const T* p = mid + plane * in_h * pitch + x0;
    int acc[kVSamples] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < taps; ++k) {
        const T* row = p + static_cast<long long>(clampi(f + k, 0, in_h - 1)) * pitch;
        const int ck = c[k];
        if constexpr (sizeof(T) == 1) {
            const uint2 q = *reinterpret_cast<const uint2*>(row);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[e] += ck * static_cast<int>((q.x >> (8 * e)) & 255u);
                acc[4 + e] += ck * static_cast<int>((q.y >> (8 * e)) & 255u);
            }
        } else {
            const uint4 q = *reinterpret_cast<const uint4*>(row);
            const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[2 * e] += ck * static_cast<int>(w[e] & 65535u);
                acc[2 * e + 1] += ck * static_cast<int>(w[e] >> 16);
            }
        }
    }
    unsigned v[kVSamples];
#pragma unroll
    for (int e = 0; e < kVSamples; ++e) v[e] = static_cast<unsigned>(finish(acc[e], max_val));
    T* d = dst + plane * plane_stride + static_cast<long long>(i) * row_stride + x0;
    if (VEC_OUT && x0 + kVSamples <= out_w) {
        if constexpr (sizeof(T) == 1) {
            *reinterpret_cast<uint2*>(d) = make_uint2(v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24),
                                                      v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24));
        } else {
            *reinterpret_cast<uint4*>(d) = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
        }
    } else {
        for (int e = 0; e < kVSamples && x0 + e < out_w; ++e) d[e] = static_cast<T>(v[e]);
    }
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int mid_pitch(int out_w) { return (out_w + kAlign - 1) / kAlign * kAlign; }

// samples a row of a horizontal tile needs in LDS, from the multiple of kAlign at or below its first tap; -1: `first` decreases
int h_span(const std::vector<int32_t>& first, int n_out, int taps)
{
    int span = 0;
    for (int j0 = 0; j0 < n_out; j0 += kHTile) {
        const int jl = std::min(j0 + kHTile, n_out) - 1;
        for (int j = j0; j < jl; ++j) {
            if (first[j + 1] < first[j]) return -1;
        }
        const int f0 = first[j0];
        const int base = (f0 >= 0 ? f0 / kAlign : -((-f0 + kAlign - 1) / kAlign)) * kAlign;
        span = std::max(span, first[jl] + taps - base);
    }
    return (span + kAlign - 1) / kAlign * kAlign;
}

template <typename T>
void launch(const ResamplePlan& p, const ResampleDesc& d, T* mid, hipStream_t stream)
{
    const T* src = static_cast<const T*>(d.src);
    T* dst = static_cast<T*>(d.dst);
    const int pitch = mid_pitch(p.out_w);
    const bool one = d.n_planes == 1;
    const bool vec_in = aligned(src, 16) && (d.src_row_stride * sizeof(T)) % 16 == 0 && (one || (d.src_plane_stride * sizeof(T)) % 16 == 0);
    const size_t vs = kVSamples * sizeof(T);
    const bool vec_out = aligned(dst, vs) && (d.dst_row_stride * sizeof(T)) % vs == 0 && (one || (d.dst_plane_stride * sizeof(T)) % vs == 0);
    const dim3 hgrid((p.out_w + kHTile - 1) / kHTile, (p.in_h + kHRows - 1) / kHRows, d.n_planes);
    const size_t lds = static_cast<size_t>(p.taps_w) * kHTile * 2 + static_cast<size_t>(kHRows) * p.span_w * sizeof(T);
    auto hk = vec_in ? resample_h_kernel<T, true> : resample_h_kernel<T, false>;
    hipLaunchKernelGGL(hk, hgrid, dim3(kThreads), lds, stream, src, static_cast<long long>(d.src_row_stride), d.src_plane_stride,
                       p.in_h, p.in_w, mid, pitch, p.out_w, p.coef_w, p.first_w, p.taps_w, p.span_w, d.max_val);
    hip_check(hipGetLastError(), "resample horizontal launch");
    const dim3 vgrid((p.out_w + 64 * kVSamples - 1) / (64 * kVSamples), (p.out_h + kVRows - 1) / kVRows, d.n_planes);
    auto vk = vec_out ? resample_v_kernel<T, true> : resample_v_kernel<T, false>;
    hipLaunchKernelGGL(vk, vgrid, dim3(kThreads), 0, stream, mid, pitch, p.in_h, dst, static_cast<long long>(d.dst_row_stride),
                       d.dst_plane_stride, p.out_h, p.out_w, p.coef_h, p.first_h, p.taps_h, d.max_val);
    hip_check(hipGetLastError(), "resample vertical launch");
}

// [lo, hi) in bytes of n planes of h rows of w samples
void extent(const void* p, int es, int n, int h, int w, long long row_stride, long long plane_stride, uintptr_t& lo, uintptr_t& hi)
{
    lo = reinterpret_cast<uintptr_t>(p);
    hi = lo + static_cast<uintptr_t>((n - 1) * plane_stride + (h - 1) * row_stride + w) * static_cast<uintptr_t>(es);
}

}  // namespace

int resample_ntaps(int n_in, int n_out)
{
    if (n_in < 1 || n_out < 1 || n_in > kResampleMaxSide || n_out > kResampleMaxSide) return -1;
    if (n_in > kResampleMaxRatio * n_out || n_out > kResampleMaxRatio * n_in) return -1;
    const double scale = static_cast<double>(n_in) / static_cast<double>(n_out);
    const double fs = scale > 1.0 ? scale : 1.0;
    const int taps = 2 * static_cast<int>(std::ceil(3.0 * fs));
    return taps <= kResampleMaxTaps ? taps : -1;
}

void resample_taps(int n_in, int n_out, int16_t* coef, int32_t* first)
{
    if (coef == nullptr || first == nullptr) throw std::invalid_argument("resample_taps: null operand");
    const int taps = resample_ntaps(n_in, n_out);
    if (taps < 0) {
        throw std::invalid_argument("resample: lengths must be in 1.." + std::to_string(kResampleMaxSide) + " at a ratio in [1/8, 8], got " +
                                    std::to_string(n_in) + " -> " + std::to_string(n_out));
    }
    const double scale = static_cast<double>(n_in) / static_cast<double>(n_out);
    const double fs = scale > 1.0 ? scale : 1.0;
    const double support = 3.0 * fs;
    double w[kResampleMaxTaps];
    for (int j = 0; j < n_out; ++j) {
        const double centre = (static_cast<double>(j) + 0.5) * scale - 0.5;
        const int f = static_cast<int>(std::floor(centre - support)) + 1;
        double sum = 0.0;
        for (int k = 0; k < taps; ++k) {
            w[k] = lanczos3((static_cast<double>(f + k) - centre) / fs);
            sum = sum + w[k];
        }
        int16_t* c = coef + static_cast<size_t>(j) * taps;
        int total = 0, best = 0, abs_sum = 0;
        int v[kResampleMaxTaps];
        for (int k = 0; k < taps; ++k) {
            v[k] = static_cast<int>(std::nearbyint(w[k] * 4096.0 / sum));      // round half to even (the default mode), as numpy's rint
            total += v[k];
            if (v[k] > v[best]) best = k;
        }
        v[best] += 4096 - total;
        for (int k = 0; k < taps; ++k) abs_sum += v[k] < 0 ? -v[k] : v[k];
        if (abs_sum > kMaxAbsCoefSum) throw std::invalid_argument("resample: a coefficient row is too large for the 32-bit accumulator");
        for (int k = 0; k < taps; ++k) c[k] = static_cast<int16_t>(v[k]);
        first[j] = f;
    }
}

ResamplePlan* resample_plan_create(int in_h, int in_w, int out_h, int out_w)
{
    const int tw = resample_ntaps(in_w, out_w), th = resample_ntaps(in_h, out_h);
    if (tw < 0 || th < 0) {
        throw std::invalid_argument("resample: sides must be in 1.." + std::to_string(kResampleMaxSide) + " and each side's ratio in [1/8, 8], got " +
                                    std::to_string(in_w) + "x" + std::to_string(in_h) + " -> " + std::to_string(out_w) + "x" + std::to_string(out_h));
    }
    std::vector<int16_t> cw(static_cast<size_t>(out_w) * tw), ch(static_cast<size_t>(out_h) * th);
    std::vector<int32_t> fw(out_w), fh(out_h);
    resample_taps(in_w, out_w, cw.data(), fw.data());
    resample_taps(in_h, out_h, ch.data(), fh.data());
    const int span = h_span(fw, out_w, tw);
    if (span < 0 || span > kMaxHSpan) throw std::runtime_error("resample: a horizontal tile does not fit its LDS segment");
    // one allocation: the int32 tables first, then the int16 ones
    const size_t b_fw = fw.size() * 4, b_fh = fh.size() * 4, b_cw = cw.size() * 2, b_ch = ch.size() * 2;
    char* dev = nullptr;
    hip_check(hipMalloc(reinterpret_cast<void**>(&dev), b_fw + b_fh + b_cw + b_ch), "hipMalloc(resample tables)");
    std::vector<char> host(b_fw + b_fh + b_cw + b_ch);
    std::memcpy(host.data(), fw.data(), b_fw);
    std::memcpy(host.data() + b_fw, fh.data(), b_fh);
    std::memcpy(host.data() + b_fw + b_fh, cw.data(), b_cw);
    std::memcpy(host.data() + b_fw + b_fh + b_cw, ch.data(), b_ch);
    const hipError_t e = hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(dev);
        hip_check(e, "hipMemcpy(resample tables)");
    }
    ResamplePlan* p = new ResamplePlan;
    p->in_h = in_h; p->in_w = in_w; p->out_h = out_h; p->out_w = out_w;
    p->taps_w = tw; p->taps_h = th; p->span_w = span;
    p->tables = dev;
    p->first_w = reinterpret_cast<const int32_t*>(dev);
    p->first_h = reinterpret_cast<const int32_t*>(dev + b_fw);
    p->coef_w = reinterpret_cast<const int16_t*>(dev + b_fw + b_fh);
    p->coef_h = reinterpret_cast<const int16_t*>(dev + b_fw + b_fh + b_cw);
    return p;
}

void resample_plan_free(ResamplePlan* p)
{
    if (p == nullptr) return;
    if (p->tables) hip_check(hipFree(p->tables), "hipFree(resample tables)");
    delete p;
}

unsigned long long resample_workspace_bytes(const ResamplePlan& p, int n_planes)
{
    // the intermediate planes [n_planes][in_h][pitch], sized for 16-bit samples, plus the slack to start them on 16 bytes
    return static_cast<unsigned long long>(n_planes) * p.in_h * mid_pitch(p.out_w) * 2 + 16;
}

void resample_validate(const ResamplePlan& p, const ResampleDesc& d)
{
    if (d.src == nullptr || d.dst == nullptr || d.workspace == nullptr) throw std::invalid_argument("resample: null operand");
    if ((d.src_dtype != kSampleU8 && d.src_dtype != kSampleU16) || d.dst_dtype != d.src_dtype) {
        throw std::invalid_argument("resample: sample types must be DCVC_SAMPLE_U8 or DCVC_SAMPLE_U16, the same on both sides");
    }
    const int es = d.src_dtype == kSampleU8 ? 1 : 2;
    if (d.max_val < 1 || d.max_val > (es == 1 ? 255 : 65535)) {
        throw std::invalid_argument("resample: max_val must be in 1..255 (u8) or 1..65535 (u16), got " + std::to_string(d.max_val));
    }
    if (d.n_planes < 1 || d.n_planes > 65535) throw std::invalid_argument("resample: n_planes must be in 1..65535");
    if (d.src_row_stride < p.in_w || d.dst_row_stride < p.out_w) throw std::invalid_argument("resample: a row stride is below the width");
    if (d.n_planes > 1 && (d.src_plane_stride < static_cast<long long>(p.in_h - 1) * d.src_row_stride + p.in_w ||
                           d.dst_plane_stride < static_cast<long long>(p.out_h - 1) * d.dst_row_stride + p.out_w)) {
        throw std::invalid_argument("resample: a plane stride is below the plane");
    }
    if (!aligned(d.src, es) || !aligned(d.dst, es)) throw std::invalid_argument("resample: 16-bit planes must be 2-byte aligned");
    if (d.workspace_bytes < 0 || static_cast<unsigned long long>(d.workspace_bytes) < resample_workspace_bytes(p, d.n_planes)) {
        throw std::invalid_argument("resample: workspace smaller than dcvc_resample_workspace_bytes");
    }
    uintptr_t s0, s1, d0, d1;
    extent(d.src, es, d.n_planes, p.in_h, p.in_w, d.src_row_stride, d.src_plane_stride, s0, s1);
    extent(d.dst, es, d.n_planes, p.out_h, p.out_w, d.dst_row_stride, d.dst_plane_stride, d0, d1);
    if (s0 < d1 && d0 < s1) throw std::invalid_argument("resample: dst overlaps src");
    const uintptr_t w0 = reinterpret_cast<uintptr_t>(d.workspace), w1 = w0 + static_cast<uintptr_t>(d.workspace_bytes);
    if ((w0 < s1 && s0 < w1) || (w0 < d1 && d0 < w1)) throw std::invalid_argument("resample: the workspace overlaps src or dst");
}

void resample_planes(const ResamplePlan& p, const ResampleDesc& d, hipStream_t stream)
{
    resample_validate(p, d);
    void* mid = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(d.workspace) + 15) & ~static_cast<uintptr_t>(15));
    if (d.src_dtype == kSampleU8) launch<uint8_t>(p, d, static_cast<uint8_t*>(mid), stream);
    else launch<uint16_t>(p, d, static_cast<uint16_t*>(mid), stream);
}

}  // namespace dcvc
