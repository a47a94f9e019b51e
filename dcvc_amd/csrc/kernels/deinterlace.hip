// deinterlace.hip - a motion-adaptive, edge-directed deinterlacer over planes of integer samples. Every output
// sample is defined exactly, in signed 32-bit integers, so a numpy restatement (tests/deinterlace_np.py) can be held against
// it with ==.
//
// Per plane, T = threshold << (bit_depth - 8); cur is the woven frame, prev the previous input frame (or none):
//   kept rows (y % 2 == keep): out[y] = cur[y].
//   missing rows: ya = y - 1 (y + 1 at the top), yb = y + 1 (y - 1 at the bottom), A = cur[ya], B = cur[yb], columns clamped.
//     spatial: for d in 0, -1, +1: score_d = sum over j in -1..1 of |A[x + j + d] - B[x + j - d]|, pred_d = (A[x + d] + B[x - d]
//              + 1) >> 1; the smallest score wins, a later direction only when strictly smaller; sp = pred_best.
//     without prev, or with T == 0: out = sp. Otherwise
//     m = max over rows {ya, y, yb} and columns x - 1 .. x + 1 of |cur - prev|, k = (256 max(0, T - m)) / T (0..256),
//     wv = prev[y][x] (weave_from_prev) or cur[y][x], out = sp + ((k (wv - sp) + 128) >> 8), the shift arithmetic.
//   sp is a rounded mean of two samples read and out lies between sp and wv: there is no clamp to max_val.
//
// The bounds: T <= 64 << 8 = 2^14, so 256 T <= 2^22 (static_assert below): the dividend is exact in fp32, the quotient at most
// 256, and floor_div takes it from one fp32 reciprocal - off by less than 256 * 2^-22 - and settles it with one exact
// remainder step each way. k <= 256 and |wv - sp| < 2^16, so |k (wv - sp)| < 2^24 and both factors fit __mul24.
//
// One launch a call: planes of one size ride in blockIdx.z, plane offsets are 64-bit. A workgroup of 256 threads makes a tile
// of kTW x kTH outputs. It stages rows y0 - 1 .. y0 + kTH of cur (and of prev) in LDS as 16-bit words for either sample type,
// the column clamp and the ya / yb rule (row -1 reads row 1, row H reads row H - 2) applied while staging, in 16-byte loads
// where the operands allow (VEC_IN) and sample by sample otherwise; a staged row starts one 16-byte vector left of the tile,
// so every vector is aligned. Without prev the missing rows of cur are not read at all. A thread then walks down one column
// of 4 missing rows: B of one row is A of the next, and so is the row's share of m, so a missing sample costs 5 LDS reads
// without prev and 14 with it. The results pass through LDS once more so that a thread stores 8 consecutive samples - of a
// kept row straight from the staged tile - as one 8- or 16-byte word (VEC_OUT). Nothing is written past W.
#include "ops.h"

#include <string>

namespace dcvc {

namespace {

constexpr int kThreads = 256;
constexpr int kTW = 128;                     // outputs of a tile along x
constexpr int kTH = 16;                      // ... and along y
constexpr int kOut = 8;                      // consecutive samples a thread stores
constexpr int kWalk = 4;                     // missing rows a thread walks down
constexpr int kMaxThreshold = 64;
static_assert(kTW * kTH == kThreads * kOut, "one store of kOut samples per thread");
static_assert(kThreads % kTW == 0 && (kThreads / kTW) * kWalk * 2 == kTH && kTH % 2 == 0, "a thread per column and kWalk missing rows");
static_assert(256LL * (static_cast<long long>(kMaxThreshold) << 8) <= (1LL << 22), "256 T must be exact in fp32");
static_assert(256LL * 65535 < (1LL << 24), "k (wv - sp) is a 24-bit product");

template <typename T> struct Vec16;                                     // a 16-byte vector's worth of samples
template <> struct Vec16<uint8_t> { static constexpr int n = 16; };
template <> struct Vec16<uint16_t> { static constexpr int n = 8; };

template <typename T> struct Tile {
    static constexpr int V = Vec16<T>::n;
    static constexpr int pitch = kTW + 2 * V;            // a staged row: one vector left of the tile, one right
    static constexpr int chunks = kTW / V + 2;
    static constexpr int rows = kTH + 2;
    static constexpr int words = rows * pitch, res_words = kTH / 2 * kTW;
    static_assert(kTW % V == 0 && V >= 2 && pitch % 8 == 0, "the two halo columns lie inside the vector on either side; rows stay 16-byte aligned");
    static_assert((2 * words + res_words) * 2 <= 64 * 1024, "the tile must fit the LDS");
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ int sad(int a, int b, int acc) { return static_cast<int>(__usad(a, b, acc)); }

// floor(a / b) for 0 <= a <= 2^22, b > 0 and a / b <= 256 (see the head of the file)
__device__ __forceinline__ int floor_div(int a, int b)
{
    int q = static_cast<int>(floorf(static_cast<float>(a) * __builtin_amdgcn_rcpf(static_cast<float>(b))));
    int r = a - __mul24(q, b);
    if (r < 0) { --q; r += b; }
    if (r >= b) ++q;
    return q;
}

// rows [y0 - 1, y0 + kTH] x columns [x0 - V, x0 + kTW + V) of a plane -> LDS: columns clamped, row -1 reads row 1 and row H
// reads row H - 2 (the ya / yb rule; rows further out are never used and only kept inside the plane). Rows of parity `skip`
// (0, 1; -1: none) are left out.
template <typename T, bool VEC>
__device__ __forceinline__ void stage(const T* __restrict__ plane, long long row_stride, int H, int W, int y0, int x0, int skip, uint16_t* lds)
{
    constexpr int V = Tile<T>::V, chunks = Tile<T>::chunks, pitch = Tile<T>::pitch;
    for (int i = threadIdx.x; i < Tile<T>::rows * chunks; i += kThreads) {
        const int r = i / chunks, c = i - r * chunks;
        int rr = y0 - 1 + r;
        if ((rr & 1) == skip) continue;
        rr = rr < 0 ? -rr : (rr >= H ? 2 * (H - 1) - rr : rr);
        const int g = x0 - V + c * V;
        const T* row = plane + static_cast<long long>(clampi(rr, 0, H - 1)) * row_stride;
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

// max over columns -1 .. 1 of |cur - prev| at one staged position
__device__ __forceinline__ int motion3(const uint16_t* c, const uint16_t* p)
{
    return max(max(sad(c[-1], p[-1], 0), sad(c[0], p[0], 0)), sad(c[1], p[1], 0));
}

template <typename T, bool HAS_PREV, bool VEC_IN, bool VEC_OUT>
__global__ void __launch_bounds__(kThreads)
deinterlace_kernel(const T* __restrict__ cur, long long cur_row_stride, long long cur_plane_stride, const T* __restrict__ prev,
                   long long prev_row_stride, long long prev_plane_stride, T* __restrict__ dst, long long dst_row_stride,
                   long long dst_plane_stride, int H, int W, int keep, int weave_from_prev, int Tm)
{
    using TL = Tile<T>;
    constexpr int V = TL::V, pitch = TL::pitch;
    __shared__ __attribute__((aligned(16))) uint16_t lds[TL::words + TL::res_words + (HAS_PREV ? TL::words : 0)];
    uint16_t* ss = lds;                                  // [kTH + 2][pitch]: cur rows y0 - 1 .., columns x0 - V ..
    uint16_t* res = lds + TL::words;                     // [kTH / 2][kTW]: the missing rows' results
    uint16_t* ps = res + TL::res_words;                  // [kTH + 2][pitch]: prev, as cur
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;      // y0 is even: a tile row's parity is the picture row's
    const long long plane = blockIdx.z;
    // without prev the missing rows are never read
    stage<T, VEC_IN>(cur + plane * cur_plane_stride, cur_row_stride, H, W, y0, x0, HAS_PREV ? -1 : 1 - keep, ss);
    if constexpr (HAS_PREV) stage<T, VEC_IN>(prev + plane * prev_plane_stride, prev_row_stride, H, W, y0, x0, -1, ps);
    __syncthreads();
    {
        // column tc of kWalk missing rows; tile row r lies at staged row r + 1, its A at r and its B at r + 2. Columns past W and
        // rows past H hold clamped samples: they are worked on like the others and dropped by the store below
        const int tc = tid % kTW, r0 = (tid / kTW) * (2 * kWalk) + (1 - keep);
        const uint16_t* s = ss + r0 * pitch + (V + tc);
        const uint16_t* p = ps + r0 * pitch + (V + tc);
        int a[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) a[j] = s[j - 2];
        int ma = 0;
        if constexpr (HAS_PREV) ma = motion3(s, p);
#pragma unroll
        for (int it = 0; it < kWalk; ++it) {
            int b[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) b[j] = s[2 * pitch + j - 2];
            // d = 0, then -1, then +1: a later direction wins only with a strictly smaller score
            int score = sad(a[1], b[1], sad(a[2], b[2], sad(a[3], b[3], 0)));
            int sp = (a[2] + b[2] + 1) >> 1;
            const int sm = sad(a[0], b[2], sad(a[1], b[3], sad(a[2], b[4], 0)));
            if (sm < score) { score = sm; sp = (a[1] + b[3] + 1) >> 1; }
            const int sq = sad(a[2], b[0], sad(a[3], b[1], sad(a[4], b[2], 0)));
            if (sq < score) sp = (a[3] + b[1] + 1) >> 1;
            int out = sp;
            if constexpr (HAS_PREV) {
                const int mb = motion3(s + 2 * pitch, p + 2 * pitch);
                const int m = max(max(ma, mb), motion3(s + pitch, p + pitch));
                const int k = floor_div(max(0, Tm - m) << 8, Tm);
                const int wv = weave_from_prev ? p[pitch] : s[pitch];
                out = sp + ((__mul24(k, wv - sp) + 128) >> 8);
                ma = mb;
            }
            res[((r0 >> 1) + it) * kTW + tc] = static_cast<uint16_t>(out);
#pragma unroll
            for (int j = 0; j < 5; ++j) a[j] = b[j];
            s += 2 * pitch;
            p += 2 * pitch;
        }
    }
    __syncthreads();
    const int r = tid / (kTW / kOut), xo = (tid - r * (kTW / kOut)) * kOut;
    const int y = y0 + r, x = x0 + xo;
    if (y >= H || x >= W) return;
    const uint16_t* from = (r & 1) == keep ? ss + (r + 1) * pitch + (V + xo) : res + (r >> 1) * kTW + xo;
    const uint4 q = *reinterpret_cast<const uint4*>(from);
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
void launch(const DeinterlaceDesc& d, hipStream_t stream)
{
    const T* cur = static_cast<const T*>(d.cur);
    const T* prev = HAS_PREV ? static_cast<const T*>(d.prev) : nullptr;
    T* dst = static_cast<T*>(d.dst);
    const bool one = d.n_planes == 1;
    auto fits = [&](const void* p, long long row_stride, long long plane_stride, size_t a) {
        return aligned(p, a) && (row_stride * sizeof(T)) % a == 0 && (one || (plane_stride * sizeof(T)) % a == 0);
    };
    const bool vec_in = fits(cur, d.cur_row_stride, d.cur_plane_stride, 16) && (!HAS_PREV || fits(prev, d.prev_row_stride, d.prev_plane_stride, 16));
    const bool vec_out = fits(dst, d.dst_row_stride, d.dst_plane_stride, kOut * sizeof(T));
    const dim3 grid((d.W + kTW - 1) / kTW, (d.H + kTH - 1) / kTH, d.n_planes);
    auto k = vec_in ? (vec_out ? deinterlace_kernel<T, HAS_PREV, true, true> : deinterlace_kernel<T, HAS_PREV, true, false>)
                    : (vec_out ? deinterlace_kernel<T, HAS_PREV, false, true> : deinterlace_kernel<T, HAS_PREV, false, false>);
    hipLaunchKernelGGL(k, grid, dim3(kThreads), 0, stream, cur, static_cast<long long>(d.cur_row_stride), d.cur_plane_stride, prev,
                       HAS_PREV ? static_cast<long long>(d.prev_row_stride) : 0LL, HAS_PREV ? d.prev_plane_stride : 0LL, dst,
                       static_cast<long long>(d.dst_row_stride), d.dst_plane_stride, d.H, d.W, d.keep, d.weave_from_prev,
                       d.threshold << (d.bit_depth - 8));
    hip_check(hipGetLastError(), "deinterlace launch");
}

}  // namespace

void deinterlace_validate(const DeinterlaceDesc& d)
{
    if (d.cur == nullptr || d.dst == nullptr) throw std::invalid_argument("deinterlace: null operand");
    if (d.dtype != kSampleU8 && d.dtype != kSampleU16) {
        throw std::invalid_argument("deinterlace: the sample type must be DCVC_SAMPLE_U8 or DCVC_SAMPLE_U16");
    }
    const int es = d.dtype == kSampleU8 ? 1 : 2;
    if (es == 1 ? d.bit_depth != 8 : (d.bit_depth < 9 || d.bit_depth > 16)) {
        throw std::invalid_argument("deinterlace: bit_depth must be 8 (u8) or 9..16 (u16), got " + std::to_string(d.bit_depth));
    }
    if (d.H < 2 || d.H > kDeinterlaceMaxSide || d.W < 1 || d.W > kDeinterlaceMaxSide) {
        throw std::invalid_argument("deinterlace: H must be in 2.." + std::to_string(kDeinterlaceMaxSide) + " and W in 1.." +
                                    std::to_string(kDeinterlaceMaxSide) + ", got " + std::to_string(d.W) + "x" + std::to_string(d.H));
    }
    if (d.n_planes < 1 || d.n_planes > 65535) throw std::invalid_argument("deinterlace: n_planes must be in 1..65535");
    if (d.keep < 0 || d.keep > 1) throw std::invalid_argument("deinterlace: keep must be 0 or 1, got " + std::to_string(d.keep));
    if (d.weave_from_prev < 0 || d.weave_from_prev > 1) {
        throw std::invalid_argument("deinterlace: weave_from_prev must be 0 or 1, got " + std::to_string(d.weave_from_prev));
    }
    if (d.threshold < 0 || d.threshold > kMaxThreshold) {
        throw std::invalid_argument("deinterlace: threshold must be in 0..64, got " + std::to_string(d.threshold));
    }
    const long long plane = static_cast<long long>(d.H - 1);
    if (d.cur_row_stride < d.W || d.dst_row_stride < d.W || (d.prev && d.prev_row_stride < d.W)) {
        throw std::invalid_argument("deinterlace: a row stride is below the width");
    }
    if (d.n_planes > 1 && (d.cur_plane_stride < plane * d.cur_row_stride + d.W || d.dst_plane_stride < plane * d.dst_row_stride + d.W ||
                           (d.prev && d.prev_plane_stride < plane * d.prev_row_stride + d.W))) {
        throw std::invalid_argument("deinterlace: a plane stride is below the plane");
    }
    if (!aligned(d.cur, es) || !aligned(d.dst, es) || !aligned(d.prev, es)) {
        throw std::invalid_argument("deinterlace: 16-bit planes must be 2-byte aligned");
    }
    uintptr_t c0, c1, d0, d1;
    extent(d.cur, es, d.n_planes, d.H, d.W, d.cur_row_stride, d.cur_plane_stride, c0, c1);
    extent(d.dst, es, d.n_planes, d.H, d.W, d.dst_row_stride, d.dst_plane_stride, d0, d1);
    if (c0 < d1 && d0 < c1) throw std::invalid_argument("deinterlace: dst overlaps cur");
    if (d.prev) {
        uintptr_t p0, p1;
        extent(d.prev, es, d.n_planes, d.H, d.W, d.prev_row_stride, d.prev_plane_stride, p0, p1);
        if (p0 < d1 && d0 < p1) throw std::invalid_argument("deinterlace: dst overlaps prev");
    }
}

void deinterlace_planes(const DeinterlaceDesc& d, hipStream_t stream)
{
    deinterlace_validate(d);
    const bool history = d.prev != nullptr && d.threshold > 0;      // without either, out = sp
    if (d.dtype == kSampleU8) {
        if (history) launch<uint8_t, true>(d, stream); else launch<uint8_t, false>(d, stream);
    } else {
        if (history) launch<uint16_t, true>(d, stream); else launch<uint16_t, false>(d, stream);
    }
}

}  // namespace dcvc
