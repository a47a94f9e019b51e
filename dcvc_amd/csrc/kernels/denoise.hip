// denoise.hip - a temporal-spatial denoising prefilter over planes of integer samples. Every output sample is
// defined exactly, in signed 32-bit integers, so a numpy restatement (tests/denoise_np.py) can be held against it with ==.
//
// Per plane, sh = bit_depth - 8, Ts = spatial << sh, Tt = temporal << sh; indexes are clamped to the plane (edge replication):
//   spatial:  c the centre, n_i the 9 samples of its 3x3 neighbourhood, w_i = max(0, Ts - |n_i - c|),
//             num = sum w_i (n_i - c), ws = sum w_i (>= Ts: the centre), sp = c + floor((2 num + ws) / (2 ws)); Ts == 0: sp = c.
//   temporal: prev the same plane of the previous OUTPUT picture; without one, or with Tt == 0, out = sp. Else
//             m = sum over the 3x3 neighbourhood q of |sp[q] - prev[q]|, L = 9 Tt, k = (192 max(0, L - m)) / L (0..192),
//             out = sp + ((k (prev - sp) + 128) >> 8), the shift arithmetic.
//   sp at a clamped index is the sp of the clamped position, not a spatial stage evaluated outside the plane.
//   Both stages give values between the smallest and the largest sample they read: there is no clamp to max_val.
//
// The accumulators: w_i |n_i - c| = (Ts - d) d <= Ts^2 / 4, and the centre's term is 0, so |num| <= 8 Ts^2 / 4 = 2 Ts^2;
// ws <= 9 Ts. At the largest Ts (64 << 8 = 16384): |2 num + ws| <= 4 * 16384^2 + 9 * 16384 < 2^31 (static_assert below).
// 192 (L - m) <= 192 * 9 * 16384 and k |prev - sp| + 128 <= 192 * 65535 + 128 are far below it.
//
// The two divisions have a positive divisor and a quotient of at most 16384 in magnitude (|num / ws| is a weighted mean of
// |n_i - c| < Ts), so floor_div takes the quotient from one fp32 reciprocal - off by less than 16384 * 2^-22 - and settles it
// with one exact remainder step each way.
//
// One launch a call: planes of one size ride in blockIdx.z, plane offsets are 64-bit. A workgroup of 256 threads makes a tile
// of kTW x kTH outputs. It stages the source tile with a 2-sample halo and prev with a 1-sample halo in LDS (16-bit words for
// either sample type), the clamp applied while staging, in 16-byte loads where the operands allow (VEC_IN) and sample by
// sample otherwise; a staged row starts one 16-byte vector left of the tile, so every vector is aligned. Then sp for the tile
// plus a 1-sample halo goes to LDS - a halo position outside the plane takes the sp of the clamped position - with
// |sp - prev| beside it, and the temporal stage sums the 9 differences and reads sp and prev from there. Threads run along
// x in every stage (conflict-free 2-byte LDS accesses); the results pass through LDS once more so that a thread stores 8
// consecutive samples as one 8- or 16-byte word (VEC_OUT).
// Nothing is written past W. Without prev (or with temporal == 0) the halo of sp, prev's tile and the temporal stage drop out.
#include "ops.h"

#include <string>

namespace dcvc {

namespace {

constexpr int kThreads = 256;
constexpr int kTW = 128;                     // outputs of a tile along x
constexpr int kTH = 16;                      // ... and along y
constexpr int kOut = 8;                      // consecutive samples a thread stores
constexpr int kMaxStrength = 64;
static_assert(kTW * kTH == kThreads * kOut, "one store of kOut samples per thread");
static_assert(kThreads % kTW == 0 && kThreads >= 2 * (kTH + 2), "threads along x, whole rows a pass; the halo's two columns in one pass");
constexpr long long kMaxT = static_cast<long long>(kMaxStrength) << 8;
static_assert(4 * kMaxT * kMaxT + 9 * kMaxT < (1LL << 31), "2 num + ws must fit the 32-bit accumulator");

template <typename T> struct Vec16;                                     // a 16-byte vector's worth of samples
template <> struct Vec16<uint8_t> { static constexpr int n = 16; };
template <> struct Vec16<uint16_t> { static constexpr int n = 8; };

template <typename T> struct Tile {
    static constexpr int V = Vec16<T>::n;
    static constexpr int pitch = kTW + 2 * V;            // a staged row: one vector left of the tile, one right
    static constexpr int chunks = kTW / V + 2;
    static constexpr int src_rows = kTH + 4, prev_rows = kTH + 2;
    static constexpr int sp_pitch = kTW + 2, sp_rows = kTH + 2;
    static constexpr int src_words = src_rows * pitch, prev_words = prev_rows * pitch, sp_words = (sp_rows * sp_pitch + 7) / 8 * 8;
    static_assert(kTW % V == 0 && V >= 2, "the halo lies inside the vector on either side");
    static_assert(src_words >= kTH * kTW && prev_words >= kTH * kTW, "the results reuse a staging region");
    static_assert((src_words + prev_words + 2 * sp_words) * 2 <= 64 * 1024, "the tile must fit the LDS");
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// floor(a / b) for b > 0 and |a / b| <= 16384 (see the head of the file); q and b fit 24 bits, so q b is a full-rate multiply
__device__ __forceinline__ int floor_div(int a, int b)
{
    int q = static_cast<int>(floorf(static_cast<float>(a) * __builtin_amdgcn_rcpf(static_cast<float>(b))));
    int r = a - __mul24(q, b);
    if (r < 0) { --q; r += b; }
    if (r >= b) ++q;
    return q;
}

// rows [ya, ya + rows) x columns [x0 - V, x0 + kTW + V) of a plane -> LDS, indexes clamped
template <typename T, bool VEC>
__device__ __forceinline__ void stage(const T* __restrict__ plane, long long row_stride, int H, int W, int ya, int rows, int x0, uint16_t* lds)
{
    constexpr int V = Tile<T>::V, chunks = Tile<T>::chunks, pitch = Tile<T>::pitch;
    for (int i = threadIdx.x; i < rows * chunks; i += kThreads) {
        const int r = i / chunks, c = i - r * chunks;
        const int g = x0 - V + c * V;
        const T* row = plane + static_cast<long long>(clampi(ya + r, 0, H - 1)) * row_stride;
        uint16_t* d = lds + r * pitch + c * V;
        if (VEC && g >= 0 && g + V <= W) {
            const uint4 q = *reinterpret_cast<const uint4*>(row + g);
            if constexpr (sizeof(T) == 1) {
                const unsigned w[4] = {q.x, q.y, q.z, q.w};
                unsigned o[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[2 * e] = (w[e] & 255u) | ((w[e] & 0xff00u) << 8);
                    o[2 * e + 1] = ((w[e] >> 16) & 255u) | ((w[e] >> 24) << 16);
                }
                reinterpret_cast<uint4*>(d)[0] = make_uint4(o[0], o[1], o[2], o[3]);
                reinterpret_cast<uint4*>(d)[1] = make_uint4(o[4], o[5], o[6], o[7]);
            } else {
                *reinterpret_cast<uint4*>(d) = q;
            }
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) d[e] = static_cast<uint16_t>(row[clampi(g + e, 0, W - 1)]);
        }
    }
}

// sp of the sample at LDS position s (row pitch `pitch`) of the staged source
__device__ __forceinline__ int spatial_at(const uint16_t* s, int pitch, int Ts)
{
    const int c = s[0];
    if (Ts == 0) return c;
    int num = 0, ws = Ts;                                // the centre: w = Ts, n - c = 0
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const int n = s[dy * pitch + dx];
            const int w = Ts - min(static_cast<int>(__usad(n, c, 0u)), Ts);
            num += __mul24(w, n - c);                    // w < 2^15, |n - c| < 2^16: a full-rate 24-bit multiply
            ws += w;
        }
    }
    return c + floor_div(2 * num + ws, 2 * ws);
}

template <typename T, bool HAS_PREV, bool VEC_IN, bool VEC_OUT>
__global__ void __launch_bounds__(kThreads)
denoise_kernel(const T* __restrict__ src, long long src_row_stride, long long src_plane_stride, const T* __restrict__ prev,
               long long prev_row_stride, long long prev_plane_stride, T* __restrict__ dst, long long dst_row_stride,
               long long dst_plane_stride, int H, int W, int Ts, int Tt)
{
    using TL = Tile<T>;
    constexpr int V = TL::V, pitch = TL::pitch, sp_pitch = TL::sp_pitch;
    __shared__ __attribute__((aligned(16))) uint16_t lds[TL::src_words + TL::prev_words + (HAS_PREV ? 2 * TL::sp_words : 0)];
    uint16_t* ss = lds;                                  // [kTH + 4][pitch]: source rows y0 - 2 .., columns x0 - V ..
    uint16_t* ps = lds + TL::src_words;                  // [kTH + 2][pitch]: prev rows y0 - 1 .., the same columns
    uint16_t* sps = ps + TL::prev_words;                 // [kTH + 2][sp_pitch]: sp of rows y0 - 1 .., columns x0 - 1 ..
    uint16_t* ads = sps + TL::sp_words;                  // ... and |sp - prev| of the same positions
    uint16_t* res = HAS_PREV ? ss : ps;                  // [kTH][kTW]: the results, in a region that is free by then
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const long long plane = blockIdx.z;
    constexpr int kRows = kThreads / kTW;                // rows a pass of the workgroup covers, a thread per column
    const int tc = tid % kTW, tr = tid / kTW;
    stage<T, VEC_IN>(src + plane * src_plane_stride, src_row_stride, H, W, y0 - 2, TL::src_rows, x0, ss);
    if constexpr (HAS_PREV) stage<T, VEC_IN>(prev + plane * prev_plane_stride, prev_row_stride, H, W, y0 - 1, TL::prev_rows, x0, ps);
    __syncthreads();
    if constexpr (HAS_PREV) {
        // sp of rows y0 - 1 .. y0 + kTH, columns x0 - 1 .. x0 + kTW: a position outside the plane takes the sp of the clamped
        // one, which lies in the tile or its halo as well. Column tc of two rows a pass, then the two columns that are left
        auto halo_sp = [&](int r, int c) {
            const int cy = clampi(y0 - 1 + r, 0, H - 1), cx = clampi(x0 - 1 + c, 0, W - 1);
            const int sp = spatial_at(ss + (cy - (y0 - 2)) * pitch + (cx - x0 + V), pitch, Ts);
            sps[r * sp_pitch + c] = static_cast<uint16_t>(sp);
            // prev was staged with the same clamp, so the position's own entry is prev at the clamped position
            ads[r * sp_pitch + c] = static_cast<uint16_t>(__usad(sp, ps[r * pitch + (c - 1 + V)], 0u));
        };
        for (int r = tr; r < TL::sp_rows; r += kRows) halo_sp(r, tc);
        if (tid < 2 * TL::sp_rows) halo_sp(tid >> 1, kTW + (tid & 1));
        __syncthreads();
        const int L = 9 * Tt;
        if (x0 + tc < W) {
            for (int r = tr; r < kTH && y0 + r < H; r += kRows) {
                const uint16_t* ad = ads + (r + 1) * sp_pitch + (tc + 1);
                int m = 0;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) m += ad[dy * sp_pitch + dx];
                }
                const int sp = sps[(r + 1) * sp_pitch + (tc + 1)], pv = ps[(r + 1) * pitch + (tc + V)];
                const int k = floor_div(__mul24(192, max(0, L - m)), L);
                res[r * kTW + tc] = static_cast<uint16_t>(sp + ((__mul24(k, pv - sp) + 128) >> 8));
            }
        }
    } else {
        if (x0 + tc < W) {
            for (int r = tr; r < kTH && y0 + r < H; r += kRows) {
                res[r * kTW + tc] = static_cast<uint16_t>(spatial_at(ss + (r + 2) * pitch + (tc + V), pitch, Ts));
            }
        }
    }
    __syncthreads();
    const int r = tid / (kTW / kOut), xo = (tid - r * (kTW / kOut)) * kOut;
    const int y = y0 + r, x = x0 + xo;
    if (y >= H || x >= W) return;
    const uint4 q = *reinterpret_cast<const uint4*>(res + r * kTW + xo);
    T* d = dst + plane * dst_plane_stride + static_cast<long long>(y) * dst_row_stride + x;
    if (VEC_OUT && x + kOut <= W) {
        if constexpr (sizeof(T) == 1) {
            *reinterpret_cast<uint2*>(d) = make_uint2((q.x & 255u) | ((q.x >> 16) << 8) | ((q.y & 255u) << 16) | ((q.y >> 16) << 24),
                                                      (q.z & 255u) | ((q.z >> 16) << 8) | ((q.w & 255u) << 16) | ((q.w >> 16) << 24));
        } else {
            *reinterpret_cast<uint4*>(d) = q;
        }
    } else {
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int e = 0; e < kOut; ++e) {
            if (x + e < W) d[e] = static_cast<T>((w[e >> 1] >> (16 * (e & 1))) & 65535u);
        }
    }
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// [lo, hi) in bytes of n planes of h rows of w samples
void extent(const void* p, int es, int n, int h, int w, long long row_stride, long long plane_stride, uintptr_t& lo, uintptr_t& hi)
{
    lo = reinterpret_cast<uintptr_t>(p);
    hi = lo + static_cast<uintptr_t>((n - 1) * plane_stride + (h - 1) * row_stride + w) * static_cast<uintptr_t>(es);
}

template <typename T, bool HAS_PREV>
void launch(const DenoiseDesc& d, hipStream_t stream)
{
    const T* src = static_cast<const T*>(d.src);
    const T* prev = HAS_PREV ? static_cast<const T*>(d.prev) : nullptr;
    T* dst = static_cast<T*>(d.dst);
    const bool one = d.n_planes == 1;
    auto fits = [&](const void* p, long long row_stride, long long plane_stride, size_t a) {
        return aligned(p, a) && (row_stride * sizeof(T)) % a == 0 && (one || (plane_stride * sizeof(T)) % a == 0);
    };
    const bool vec_in = fits(src, d.src_row_stride, d.src_plane_stride, 16) && (!HAS_PREV || fits(prev, d.prev_row_stride, d.prev_plane_stride, 16));
    const bool vec_out = fits(dst, d.dst_row_stride, d.dst_plane_stride, kOut * sizeof(T));
    const int sh = d.bit_depth - 8;
    const dim3 grid((d.W + kTW - 1) / kTW, (d.H + kTH - 1) / kTH, d.n_planes);
    auto k = vec_in ? (vec_out ? denoise_kernel<T, HAS_PREV, true, true> : denoise_kernel<T, HAS_PREV, true, false>)
                    : (vec_out ? denoise_kernel<T, HAS_PREV, false, true> : denoise_kernel<T, HAS_PREV, false, false>);
    hipLaunchKernelGGL(k, grid, dim3(kThreads), 0, stream, src, static_cast<long long>(d.src_row_stride), d.src_plane_stride, prev,
                       static_cast<long long>(d.prev_row_stride), d.prev_plane_stride, dst, static_cast<long long>(d.dst_row_stride),
                       d.dst_plane_stride, d.H, d.W, d.spatial << sh, d.temporal << sh);
    hip_check(hipGetLastError(), "denoise launch");
}

}  // namespace

void denoise_validate(const DenoiseDesc& d)
{
    if (d.src == nullptr || d.dst == nullptr) throw std::invalid_argument("denoise: null operand");
    if (d.dtype != kSampleU8 && d.dtype != kSampleU16) throw std::invalid_argument("denoise: the sample type must be DCVC_SAMPLE_U8 or DCVC_SAMPLE_U16");
    const int es = d.dtype == kSampleU8 ? 1 : 2;
    if (es == 1 ? d.bit_depth != 8 : (d.bit_depth < 9 || d.bit_depth > 16)) {
        throw std::invalid_argument("denoise: bit_depth must be 8 (u8) or 9..16 (u16), got " + std::to_string(d.bit_depth));
    }
    if (d.H < 1 || d.W < 1 || d.H > kDenoiseMaxSide || d.W > kDenoiseMaxSide) {
        throw std::invalid_argument("denoise: sides must be in 1.." + std::to_string(kDenoiseMaxSide) + ", got " + std::to_string(d.W) + "x" +
                                    std::to_string(d.H));
    }
    if (d.n_planes < 1 || d.n_planes > 65535) throw std::invalid_argument("denoise: n_planes must be in 1..65535");
    if (d.spatial < 0 || d.spatial > kMaxStrength || d.temporal < 0 || d.temporal > kMaxStrength) {
        throw std::invalid_argument("denoise: strengths must be in 0..64, got " + std::to_string(d.spatial) + ":" + std::to_string(d.temporal));
    }
    const long long plane = static_cast<long long>(d.H - 1);
    if (d.src_row_stride < d.W || d.dst_row_stride < d.W || (d.prev && d.prev_row_stride < d.W)) {
        throw std::invalid_argument("denoise: a row stride is below the width");
    }
    if (d.n_planes > 1 && (d.src_plane_stride < plane * d.src_row_stride + d.W || d.dst_plane_stride < plane * d.dst_row_stride + d.W ||
                           (d.prev && d.prev_plane_stride < plane * d.prev_row_stride + d.W))) {
        throw std::invalid_argument("denoise: a plane stride is below the plane");
    }
    if (!aligned(d.src, es) || !aligned(d.dst, es) || !aligned(d.prev, es)) throw std::invalid_argument("denoise: 16-bit planes must be 2-byte aligned");
    uintptr_t s0, s1, d0, d1;
    extent(d.src, es, d.n_planes, d.H, d.W, d.src_row_stride, d.src_plane_stride, s0, s1);
    extent(d.dst, es, d.n_planes, d.H, d.W, d.dst_row_stride, d.dst_plane_stride, d0, d1);
    if (s0 < d1 && d0 < s1) throw std::invalid_argument("denoise: dst overlaps src");
    if (d.prev) {
        uintptr_t p0, p1;
        extent(d.prev, es, d.n_planes, d.H, d.W, d.prev_row_stride, d.prev_plane_stride, p0, p1);
        if (p0 < d1 && d0 < p1) throw std::invalid_argument("denoise: dst overlaps prev");
    }
}

void denoise_planes(const DenoiseDesc& d, hipStream_t stream)
{
    denoise_validate(d);
    const bool history = d.prev != nullptr && d.temporal > 0;      // without either, out = sp
    if (d.dtype == kSampleU8) {
        if (history) launch<uint8_t, true>(d, stream); else launch<uint8_t, false>(d, stream);
    } else {
        if (history) launch<uint16_t, true>(d, stream); else launch<uint16_t, false>(d, stream);
    }
}

}  // namespace dcvc
