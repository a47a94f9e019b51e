// ivtc.hip - the two device pieces of inverse telecine: field_match measures how well the second field of a
// woven luma plane fits the first field of the same frame (match c) or the second field of the previous frame fits it (match
// p), and weave_fields puts a frame together from the rows of two plane sets. Everything is an exact integer, so a numpy
// restatement (tests/ivtc_np.py) is held against both with ==.
//
// field_match. first = the parity of the rows of the field shown first, q = 1 - first, t = cthresh << (bit_depth - 8). For a
// candidate S in {cur (c), prev (p)}, over the rows y with y % 2 == q and 1 <= y <= H - 2 and every x, with a = cur[y-1][x],
// b = cur[y+1][x], s = S[y][x]:
//   match_S  = sum |2 s - a - b|
//   comb_S   = the number of samples with (s - a > t and s - b > t) or (s - a < -t and s - b < -t)
//   blkmax_S = the largest count of such samples in a block (y / 16, x / 32), blocks aligned to the plane's origin
//   dup      = sum |cur[y][x] - prev[y][x]| over ALL rows with y % 2 == first
// out8 (device, eight uint64) = [match_c, match_p, comb_c, comb_p, blkmax_c, blkmax_p, dup, 0]; without prev words 1, 3, 5 and 6
// are 0.
//
// A workgroup of 256 threads takes a tile of kTileRows rows x kVecCols 16-byte vectors; a thread walks down kRows rows of one
// vector column, holding the row above, the row itself and the row below in registers, so a plane is read once but for the one
// halo row of every kRows (the parity decides whether it lies above or below). A thread's rows lie in one block row and its
// vector in one block column: its comb counts go to the block's LDS counter, its sums through the wave (shuffles) and through
// LDS, and the workgroup issues one integer atomic per word: adds for the sums and counts, max for blkmax. Integer adds and max
// commute, so the words are the same for every launch geometry and arrival order. A first, one-workgroup launch zeroes the
// words: two launches, nothing allocated, no host wait.
//
// The bounds: one sample contributes at most 2 * 65535 to a match sum (and 65535 to dup); a workgroup sums kTileRows / 2 rows
// of kVecCols * V samples in 32 bits (static_assert in Tile below), the eight words are 64-bit: 2^14 x 2^13 rows x 2^17 < 2^45.
//
// weave_fields: dst rows of parity `first` come from plane set a, the others from b, every plane on its own; planes ride in
// blockIdx.z, offsets are 64-bit, a thread copies one 16-byte vector where the three operands allow and the vector ends inside
// W, samples otherwise. Nothing is written past W.
#include "ops.h"

#include <string>

namespace dcvc {

namespace {

constexpr int kThreads = 256;
constexpr int kVecCols = 32;                 // 16-byte vectors of a tile along x
constexpr int kRows = 8;                     // rows a thread walks down
constexpr int kTileRows = kThreads / kVecCols * kRows;
constexpr int kBlockH = 16, kBlockW = 32;    // the blocks of blkmax
constexpr int kMaxCthresh = 255;
static_assert(kThreads % kVecCols == 0 && kRows % 2 == 0 && kBlockH % kRows == 0 && kTileRows % kBlockH == 0,
              "a thread's rows lie in one block row, a tile holds whole block rows, and a row's parity is the tile row's");

template <typename T> struct Tile {
    static constexpr int V = 16 / static_cast<int>(sizeof(T));          // samples of a 16-byte vector
    static constexpr int cols = kVecCols * V;
    static constexpr int blocks_x = cols / kBlockW, blocks_y = kTileRows / kBlockH, blocks = blocks_x * blocks_y;
    static constexpr long long max_term = 2LL * (sizeof(T) == 1 ? 255 : 65535);      // |2 s - a - b|
    static_assert(kBlockW % V == 0 && cols % kBlockW == 0, "a thread's vector lies in one block column");
    static_assert(blocks <= 64, "a lane of wave 0 per block counter");
    static_assert(max_term <= 2LL * 65535, "one sample contributes at most 2 * 65535");
    static_assert(max_term * (kTileRows / 2) * cols < (1LL << 32), "a workgroup's partial sums fit 32 bits");
    static_assert((kTileRows / 2) * cols < (1 << 24) && kBlockH / 2 * kBlockW == 256, "counts: a block holds 256 measured samples");
};

// n samples (1..V) of a row from x on -> r[0..n), the rest 0; a whole vector in one 16-byte load where VEC says it is aligned
template <typename T, bool VEC>
__device__ __forceinline__ void load_row(const T* __restrict__ row, int n, int (&r)[Tile<T>::V])
{
    constexpr int V = Tile<T>::V;
    if (VEC && n == V) {
        const uint4 v = *reinterpret_cast<const uint4*>(row);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
        if constexpr (sizeof(T) == 1) {
#pragma unroll
            for (int e = 0; e < V; ++e) r[e] = static_cast<int>((w[e >> 2] >> (8 * (e & 3))) & 255u);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) r[e] = static_cast<int>((w[e >> 1] >> (16 * (e & 1))) & 65535u);
        }
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) r[e] = e < n ? static_cast<int>(row[e]) : 0;
    }
}

__device__ __forceinline__ unsigned absdiff(int a, int b) { return static_cast<unsigned>(a > b ? a - b : b - a); }

__device__ __forceinline__ unsigned combed(int s, int a, int b, int t)
{
    const int da = s - a, db = s - b;
    return ((da > t && db > t) || (da < -t && db < -t)) ? 1u : 0u;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

__global__ void field_match_zero_kernel(unsigned long long* __restrict__ out8) { out8[threadIdx.x] = 0ull; }

template <typename T, bool HAS_PREV, bool VEC>
__global__ void __launch_bounds__(kThreads)
field_match_kernel(const T* __restrict__ cur, long long cur_row_stride, const T* __restrict__ prev, long long prev_row_stride, int H, int W,
                   int first, int t, unsigned long long* __restrict__ out8)
{
    using TL = Tile<T>;
    constexpr int V = TL::V, kWaves = kThreads / 64;
    __shared__ unsigned blk[2][TL::blocks];          // comb counts of the tile's blocks: c, p
    __shared__ unsigned part[3][kWaves];             // match_c, match_p, dup of every wave
    const int tid = threadIdx.x, tx = tid % kVecCols, ty = tid / kVecCols;
    if (tid < TL::blocks) blk[0][tid] = blk[1][tid] = 0u;
    __syncthreads();
    const int x = blockIdx.x * TL::cols + tx * V, y0 = blockIdx.y * kTileRows + ty * kRows;      // y0 is even
    const int n = min(V, W - x);                     // <= 0: the vector lies past the plane
    const int q = 1 - first;
    unsigned mc = 0, mp = 0, dup = 0, cc = 0, cp = 0;
    if (n > 0 && y0 < H) {
        const T* c0 = cur + x;
        const T* p0 = HAS_PREV ? prev + x : nullptr;
        int a[V] = {}, s[V], b[V] = {}, ps[V] = {};
        // the walk: at row y, `a` holds cur[y - 1] (once y >= 1), `s` cur[y], and `b` cur[y + 1] is read for the rows that are measured
        if (y0 >= 1) load_row<T, VEC>(c0 + static_cast<long long>(y0 - 1) * cur_row_stride, n, a);
        load_row<T, VEC>(c0 + static_cast<long long>(y0) * cur_row_stride, n, s);
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int y = y0 + r;
            if (y >= H) break;
            if constexpr (HAS_PREV) load_row<T, VEC>(p0 + static_cast<long long>(y) * prev_row_stride, n, ps);
            const bool more = y + 1 < H;
            if (more) load_row<T, VEC>(c0 + static_cast<long long>(y + 1) * cur_row_stride, n, b);
            if ((y & 1) == q) {
                if (y >= 1 && more) {
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        if (e < n) {
                            mc += absdiff(2 * s[e], a[e] + b[e]);
                            cc += combed(s[e], a[e], b[e], t);
                            if constexpr (HAS_PREV) {
                                mp += absdiff(2 * ps[e], a[e] + b[e]);
                                cp += combed(ps[e], a[e], b[e], t);
                            }
                        }
                    }
                }
            } else if constexpr (HAS_PREV) {
#pragma unroll
                for (int e = 0; e < V; ++e) dup += absdiff(s[e], ps[e]);      // samples past n are 0 in both
            }
#pragma unroll
            for (int e = 0; e < V; ++e) { a[e] = s[e]; s[e] = b[e]; }
        }
        const int bi = (ty * kRows / kBlockH) * TL::blocks_x + tx * V / kBlockW;
        if (cc) atomicAdd(&blk[0][bi], cc);
        if (HAS_PREV && cp) atomicAdd(&blk[1][bi], cp);
    }
    mc = wave_sum(mc);
    if constexpr (HAS_PREV) { mp = wave_sum(mp); dup = wave_sum(dup); }
    if ((tid & 63) == 0) {
        part[0][tid >> 6] = mc;
        part[1][tid >> 6] = mp;
        part[2][tid >> 6] = dup;
    }
    __syncthreads();
    // wave 0: the block counters -> the tile's count and its largest block; thread 0 issues the workgroup's atomics
    if (tid < 64) {
        unsigned nc = tid < TL::blocks ? blk[0][tid] : 0u, np = tid < TL::blocks ? blk[1][tid] : 0u;
        unsigned xc = nc, xp = np;
        for (int o = 32; o > 0; o >>= 1) {
            nc += __shfl_down(nc, o);
            np += __shfl_down(np, o);
            xc = max(xc, __shfl_down(xc, o));
            xp = max(xp, __shfl_down(xp, o));
        }
        if (tid == 0) {
            unsigned tc = 0, tp = 0, td = 0;
            for (int k = 0; k < kWaves; ++k) { tc += part[0][k]; tp += part[1][k]; td += part[2][k]; }
            if (tc) atomicAdd(out8 + 0, static_cast<unsigned long long>(tc));
            if (nc) atomicAdd(out8 + 2, static_cast<unsigned long long>(nc));
            if (xc) atomicMax(out8 + 4, static_cast<unsigned long long>(xc));
            if constexpr (HAS_PREV) {
                if (tp) atomicAdd(out8 + 1, static_cast<unsigned long long>(tp));
                if (np) atomicAdd(out8 + 3, static_cast<unsigned long long>(np));
                if (xp) atomicMax(out8 + 5, static_cast<unsigned long long>(xp));
                if (td) atomicAdd(out8 + 6, static_cast<unsigned long long>(td));
            }
        }
    }
}

constexpr int kWeaveX = 64, kWeaveY = 4;     // a workgroup copies kWeaveX vectors of kWeaveY rows
static_assert(kWeaveX * kWeaveY == kThreads, "a vector per thread");

template <typename T, bool VEC>
__global__ void __launch_bounds__(kThreads)
weave_fields_kernel(const T* __restrict__ a, long long a_row_stride, long long a_plane_stride, const T* __restrict__ b, long long b_row_stride,
                    long long b_plane_stride, T* __restrict__ dst, long long dst_row_stride, long long dst_plane_stride, int H, int W, int first)
{
    constexpr int V = Tile<T>::V;
    const int x = (blockIdx.x * kWeaveX + threadIdx.x % kWeaveX) * V, y = blockIdx.y * kWeaveY + threadIdx.x / kWeaveX;
    if (x >= W || y >= H) return;
    const long long plane = blockIdx.z;
    const T* s = (y & 1) == first ? a + plane * a_plane_stride + static_cast<long long>(y) * a_row_stride + x
                                  : b + plane * b_plane_stride + static_cast<long long>(y) * b_row_stride + x;
    T* d = dst + plane * dst_plane_stride + static_cast<long long>(y) * dst_row_stride + x;
    if (VEC && x + V <= W) {
        *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
    } else {
        const int n = min(V, W - x);
        for (int e = 0; e < n; ++e) d[e] = s[e];
    }
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// [lo, hi) in bytes of n planes of h rows of w samples
void extent(const void* p, int es, int n, int h, int w, long long row_stride, long long plane_stride, uintptr_t& lo, uintptr_t& hi)
{
    lo = reinterpret_cast<uintptr_t>(p);
    hi = lo + static_cast<uintptr_t>((n - 1) * plane_stride + (h - 1) * row_stride + w) * static_cast<uintptr_t>(es);
}

// what both entries refuse alike; `who` names the kernel in the message
int sample_bytes(const char* who, int dtype, int bit_depth, bool depth_given, int H, int W)
{
    const std::string k = who;
    if (dtype != kSampleU8 && dtype != kSampleU16) throw std::invalid_argument(k + ": the sample type must be DCVC_SAMPLE_U8 or DCVC_SAMPLE_U16");
    const int es = dtype == kSampleU8 ? 1 : 2;
    if (depth_given && (es == 1 ? bit_depth != 8 : (bit_depth < 9 || bit_depth > 16))) {
        throw std::invalid_argument(k + ": bit_depth must be 8 (u8) or 9..16 (u16), got " + std::to_string(bit_depth));
    }
    if (H < 2 || H > kIvtcMaxSide || W < 1 || W > kIvtcMaxSide) {
        throw std::invalid_argument(k + ": H must be in 2.." + std::to_string(kIvtcMaxSide) + " and W in 1.." + std::to_string(kIvtcMaxSide) +
                                    ", got " + std::to_string(W) + "x" + std::to_string(H));
    }
    return es;
}

template <typename T, bool HAS_PREV>
void launch_match(const FieldMatchDesc& d, hipStream_t stream)
{
    const T* cur = static_cast<const T*>(d.cur);
    const T* prev = HAS_PREV ? static_cast<const T*>(d.prev) : nullptr;
    unsigned long long* out8 = static_cast<unsigned long long*>(d.out8);
    const bool vec = aligned(cur, 16) && (d.cur_row_stride * sizeof(T)) % 16 == 0 &&
                     (!HAS_PREV || (aligned(prev, 16) && (d.prev_row_stride * sizeof(T)) % 16 == 0));
    hipLaunchKernelGGL(field_match_zero_kernel, dim3(1), dim3(8), 0, stream, out8);
    hip_check(hipGetLastError(), "field_match zero launch");
    const dim3 grid((d.W + Tile<T>::cols - 1) / Tile<T>::cols, (d.H + kTileRows - 1) / kTileRows);
    auto k = vec ? field_match_kernel<T, HAS_PREV, true> : field_match_kernel<T, HAS_PREV, false>;
    hipLaunchKernelGGL(k, grid, dim3(kThreads), 0, stream, cur, static_cast<long long>(d.cur_row_stride), prev,
                       HAS_PREV ? static_cast<long long>(d.prev_row_stride) : 0LL, d.H, d.W, d.first, d.cthresh << (d.bit_depth - 8), out8);
    hip_check(hipGetLastError(), "field_match launch");
}

template <typename T>
void launch_weave(const WeaveFieldsDesc& d, hipStream_t stream)
{
    const bool one = d.n_planes == 1;
    auto fits = [&](const void* p, long long row_stride, long long plane_stride) {
        return aligned(p, 16) && (row_stride * sizeof(T)) % 16 == 0 && (one || (plane_stride * sizeof(T)) % 16 == 0);
    };
    const bool vec = fits(d.a, d.a_row_stride, d.a_plane_stride) && fits(d.b, d.b_row_stride, d.b_plane_stride) &&
                     fits(d.dst, d.dst_row_stride, d.dst_plane_stride);
    constexpr int V = Tile<T>::V;
    const dim3 grid((d.W + kWeaveX * V - 1) / (kWeaveX * V), (d.H + kWeaveY - 1) / kWeaveY, d.n_planes);
    auto k = vec ? weave_fields_kernel<T, true> : weave_fields_kernel<T, false>;
    hipLaunchKernelGGL(k, grid, dim3(kThreads), 0, stream, static_cast<const T*>(d.a), static_cast<long long>(d.a_row_stride), d.a_plane_stride,
                       static_cast<const T*>(d.b), static_cast<long long>(d.b_row_stride), d.b_plane_stride, static_cast<T*>(d.dst),
                       static_cast<long long>(d.dst_row_stride), d.dst_plane_stride, d.H, d.W, d.first);
    hip_check(hipGetLastError(), "weave_fields launch");
}

}  // namespace

void field_match_validate(const FieldMatchDesc& d)
{
    if (d.cur == nullptr || d.out8 == nullptr) throw std::invalid_argument("field_match: null operand");
    const int es = sample_bytes("field_match", d.dtype, d.bit_depth, true, d.H, d.W);
    if (d.first < 0 || d.first > 1) throw std::invalid_argument("field_match: first must be 0 or 1, got " + std::to_string(d.first));
    if (d.cthresh < 0 || d.cthresh > kMaxCthresh) {
        throw std::invalid_argument("field_match: cthresh must be in 0..255, got " + std::to_string(d.cthresh));
    }
    if (d.cur_row_stride < d.W || (d.prev && d.prev_row_stride < d.W)) throw std::invalid_argument("field_match: a row stride is below the width");
    if (!aligned(d.cur, es) || !aligned(d.prev, es)) throw std::invalid_argument("field_match: 16-bit planes must be 2-byte aligned");
    if (!aligned(d.out8, 8)) throw std::invalid_argument("field_match: out8 must be 8-byte aligned");
}

void field_match(const FieldMatchDesc& d, hipStream_t stream)
{
    field_match_validate(d);
    if (d.dtype == kSampleU8) {
        if (d.prev) launch_match<uint8_t, true>(d, stream); else launch_match<uint8_t, false>(d, stream);
    } else {
        if (d.prev) launch_match<uint16_t, true>(d, stream); else launch_match<uint16_t, false>(d, stream);
    }
}

void weave_fields_validate(const WeaveFieldsDesc& d)
{
    if (d.a == nullptr || d.b == nullptr || d.dst == nullptr) throw std::invalid_argument("weave_fields: null operand");
    const int es = sample_bytes("weave_fields", d.dtype, 0, false, d.H, d.W);
    if (d.n_planes < 1 || d.n_planes > 65535) throw std::invalid_argument("weave_fields: n_planes must be in 1..65535");
    if (d.first < 0 || d.first > 1) throw std::invalid_argument("weave_fields: first must be 0 or 1, got " + std::to_string(d.first));
    const long long plane = static_cast<long long>(d.H - 1);
    if (d.a_row_stride < d.W || d.b_row_stride < d.W || d.dst_row_stride < d.W) {
        throw std::invalid_argument("weave_fields: a row stride is below the width");
    }
    if (d.n_planes > 1 && (d.a_plane_stride < plane * d.a_row_stride + d.W || d.b_plane_stride < plane * d.b_row_stride + d.W ||
                           d.dst_plane_stride < plane * d.dst_row_stride + d.W)) {
        throw std::invalid_argument("weave_fields: a plane stride is below the plane");
    }
    if (!aligned(d.a, es) || !aligned(d.b, es) || !aligned(d.dst, es)) {
        throw std::invalid_argument("weave_fields: 16-bit planes must be 2-byte aligned");
    }
    uintptr_t a0, a1, b0, b1, d0, d1;
    extent(d.a, es, d.n_planes, d.H, d.W, d.a_row_stride, d.a_plane_stride, a0, a1);
    extent(d.b, es, d.n_planes, d.H, d.W, d.b_row_stride, d.b_plane_stride, b0, b1);
    extent(d.dst, es, d.n_planes, d.H, d.W, d.dst_row_stride, d.dst_plane_stride, d0, d1);
    if (a0 < d1 && d0 < a1) throw std::invalid_argument("weave_fields: dst overlaps a");
    if (b0 < d1 && d0 < b1) throw std::invalid_argument("weave_fields: dst overlaps b");
}

void weave_fields(const WeaveFieldsDesc& d, hipStream_t stream)
{
    weave_fields_validate(d);
    if (d.dtype == kSampleU8) launch_weave<uint8_t>(d, stream); else launch_weave<uint16_t>(d, stream);
}

}  // namespace dcvc
