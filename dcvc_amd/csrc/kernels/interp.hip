// interp.hip - frame-rate conversion: the picture at k / N of the way from picture A to picture B, through the vectors of
// motion_search(cur = B, ref = A). Everything is defined exactly, in signed 32-bit integers, so a numpy
// restatement (tests/interp_np.py) can be held against both kernels with ==.
//
// N in 2..8, k in 1..N-1, sh = bit_depth - 8. Blocks are 16 x 16 luma samples, Bh = ceil(H / 16), Bw = ceil(W / 16). All indexes
// into a plane are clamped to it; all divisions are floor divisions of signed integers.
//   vectors:       mv [Bh][Bw][2] holds (dx, dy) with B[p] ~ A[p + v]; each component is clamped to -31..31 when read.
//   split:         per component a = (2 k v + N) / (2 N) (k v / N rounded, halves up), b = a - v: the in-between sample at p is
//                  seen at A[p + a] and at B[p + b].
//   selection:     luma only. The candidates of block (by, bx) are the clamped vectors of the 3 x 3 neighbourhood of mv[by][bx],
//                  grid indexes clamped to [0, Bh) x [0, Bw), and (0, 0). SAD(v) = sum of |A[p + a] - B[p + b]| over the block's
//                  samples inside the plane; no penalty. The smallest tuple (SAD, |vx| + |vy|, vy, vx) wins. The block falls
//                  back when SAD > (LIMIT << sh) * n, n the number of samples summed.
//                  plan[by][bx] = (ax, ay, bx, by) and wb = k for a block that agrees; (0, 0, 0, 0) and wb = 0 (2 k <= N) or
//                  wb = N for one that fell back: it repeats the nearer picture.
//   interpolation: a plane subsampled by (sx, sy): the block of sample (y, x) is (y / (16 >> sy), x / (16 >> sx)), the offsets
//                  are ax >> sx, ay >> sy, bx >> sx, by >> sy (arithmetic shifts), w = min(wb, N),
//                  dst = ((N - w) A[y + ay][x + ax] + w B[y + by][x + bx] + (N >> 1)) / N.
//   picture rule:  with a counter `fallen` and 2 * fallen > n_blocks the interpolation treats every block as fallen.
//
// Bounds: a SAD is at most 256 * 65535 < 2^24, so the 64-bit key of motion.hip, SAD << 20 | (|vx| + |vy|) << 14 | (vy + 64) << 7 |
// (vx + 64), orders as the tuple does; (LIMIT << sh) * n <= (255 << 8) * 256 < 2^24; the blend's largest intermediate is
// 8 * 65535 + 4 < 2^20. plan and wb are device data and are not validated: the clamps make any value safe.
//
// interp_select is one launch, one wave per block. Lanes 0..8 read the neighbourhood's vectors, lane 9 holds (0, 0); a candidate
// that an earlier lane holds too is skipped (one ballot), so a block inside a uniform pan sums two candidates, not ten. Lanes
// run over the block's samples, 4 each, 16 consecutive samples of a row to 16 lanes, and read A and B straight from memory: a
// candidate reads each of its samples once, so staging them in LDS would add a pass and save none, and the union of ten windows
// (up to 78 x 78 samples a picture) is mostly samples no candidate reads. A wave sum gives the SAD to every lane; lane 0 stores
// the winner and counts a fallen block (one integer atomic).
//
// interp_planes is one launch: planes of one size ride in blockIdx.z, plane offsets are 64-bit. A workgroup of 256 threads makes
// a tile of kTW x kTH outputs, as compensate_kernel of motion.hip does. The tile lies in at most 16 x 2 blocks: their offsets,
// shifted, and weights go to LDS first, the picture rule applied there (the counter is read on the device), so the fetch loop
// reads no grid. Threads run along x while they fetch; a sample whose weight is 0 is not fetched, so a repeated block costs a
// copy. The results pass through LDS so that a thread stores 8 consecutive samples as one 8- or 16-byte word (VEC_OUT) where
// dst's base and strides allow. Nothing is written past W.
#include "ops.h"

#include <string>

namespace dcvc {

namespace {

constexpr int kB = kMotionBlock;             // luma samples a block side
static_assert(kB == 16, "the kernels shift by 4");
static_assert(256LL * 65535 < (1LL << 24) && (static_cast<long long>(kInterpMaxLimit) << 8) * 256 < (1LL << 24), "a SAD and its limit fit 24 bits");
static_assert(kInterpMaxVec < 64 && 2 * kInterpMaxVec < 64, "a component must fit 7 bits with its offset, the length 6 bits");
static_assert(kInterpMaxN * 65535LL + (kInterpMaxN >> 1) < (1LL << 20), "the blend's accumulator");

constexpr int kThreads = 256;                // the interpolation launch
constexpr int kTW = 128;
constexpr int kTH = 16;
constexpr int kOut = 8;
constexpr int kTileBW = kTW / (kB / 2);      // the blocks a tile can touch at the smallest block, 8 x 8: 16 across ...
constexpr int kTileBH = kTH / (kB / 2);      // ... and 2 down
static_assert(kTW * kTH == kThreads * kOut, "one store of kOut samples per thread");
static_assert(kTileBW * kTileBH <= kThreads, "one thread per block of the tile");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ int floordiv(int x, int d)       // d > 0
{
    const int q = x / d;
    return (x % d != 0 && x < 0) ? q - 1 : q;
}

__device__ __forceinline__ unsigned long long pack_key(int cost, int dx, int dy)
{
    return (static_cast<unsigned long long>(cost) << 20) | (static_cast<unsigned long long>(abs(dx) + abs(dy)) << 14) |
           (static_cast<unsigned long long>(dy + 64) << 7) | static_cast<unsigned long long>(dx + 64);
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// one wave per block (by, bx) = (blockIdx.y, blockIdx.x); the grid is Bh x Bw
template <typename T>
__global__ void __launch_bounds__(64)
select_kernel(const T* __restrict__ a, long long a_row_stride, const T* __restrict__ b, long long b_row_stride, int H, int W,
              const int16_t* __restrict__ mv, int mv_bw, int k, int n, unsigned limit, int16_t* __restrict__ plan,
              uint8_t* __restrict__ wb, int plan_bw, uint32_t* __restrict__ sad_out, uint32_t* __restrict__ fallen)
{
    const int lane = threadIdx.x;
    const int bx = blockIdx.x, by = blockIdx.y;
    const int Bw = gridDim.x, Bh = gridDim.y;
    int packed = -1;                                     // (vy + 64) << 7 | (vx + 64); no candidate in lanes 10..63
    if (lane < 9) {
        const int gy = clampi(by + lane / 3 - 1, 0, Bh - 1), gx = clampi(bx + lane % 3 - 1, 0, Bw - 1);
        const int16_t* v = mv + 2 * (static_cast<long long>(gy) * mv_bw + gx);
        packed = ((clampi(v[1], -kInterpMaxVec, kInterpMaxVec) + 64) << 7) | (clampi(v[0], -kInterpMaxVec, kInterpMaxVec) + 64);
    } else if (lane == 9) {
        packed = (64 << 7) | 64;
    }
    const int x0 = bx * kB, y0 = by * kB;
    const int bw0 = min(kB, W - x0), bh0 = min(kB, H - y0);
    // the samples of this lane: i = lane + 64 q, row i / 16, column i % 16
    const int col = lane & (kB - 1), row = lane >> 4;
    const int x = x0 + col;
    unsigned long long best = ~0ULL;
    for (int c = 0; c < 10; ++c) {
        const int pv = __shfl(packed, c, 64);
        const unsigned long long same = __ballot(packed == pv);
        if (__ffsll(static_cast<long long>(same)) - 1 < c) continue;      // an earlier lane holds this vector: the key would be equal
        const int vx = (pv & 127) - 64, vy = (pv >> 7) - 64;
        const int ax = floordiv(2 * k * vx + n, 2 * n), ay = floordiv(2 * k * vy + n, 2 * n);
        const int ox = ax - vx, oy = ay - vy;                             // b's offsets
        const int xa = clampi(x + ax, 0, W - 1), xb = clampi(x + ox, 0, W - 1);
        unsigned s = 0;
        if (col < bw0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = row + 4 * q;
                if (r < bh0) {
                    const int y = y0 + r;
                    const unsigned sa = a[static_cast<long long>(clampi(y + ay, 0, H - 1)) * a_row_stride + xa];
                    const unsigned sb = b[static_cast<long long>(clampi(y + oy, 0, H - 1)) * b_row_stride + xb];
                    s = __usad(sa, sb, s);
                }
            }
        }
        const int total = wave_sum(static_cast<int>(s));
        const unsigned long long key = pack_key(total, vx, vy);
        best = key < best ? key : best;
    }
    if (lane == 0) {
        const int vx = static_cast<int>(best & 127) - 64, vy = static_cast<int>((best >> 7) & 127) - 64;
        const unsigned sad = static_cast<unsigned>(best >> 20);
        const bool fell = sad > limit * static_cast<unsigned>(bw0 * bh0);
        const int ax = fell ? 0 : floordiv(2 * k * vx + n, 2 * n), ay = fell ? 0 : floordiv(2 * k * vy + n, 2 * n);
        const long long g = static_cast<long long>(by) * plan_bw + bx;
        plan[4 * g] = static_cast<int16_t>(ax);
        plan[4 * g + 1] = static_cast<int16_t>(ay);
        plan[4 * g + 2] = static_cast<int16_t>(fell ? 0 : ax - vx);
        plan[4 * g + 3] = static_cast<int16_t>(fell ? 0 : ay - vy);
        wb[g] = static_cast<uint8_t>(fell ? (2 * k <= n ? 0 : n) : k);
        if (sad_out) sad_out[g] = sad;
        if (fell && fallen) atomicAdd(fallen, 1u);
    }
}

template <typename T, bool VEC_OUT>
__global__ void __launch_bounds__(kThreads)
interp_kernel(const T* __restrict__ a, long long a_row_stride, long long a_plane_stride, const T* __restrict__ b, long long b_row_stride,
              long long b_plane_stride, T* __restrict__ dst, long long dst_row_stride, long long dst_plane_stride, int H, int W, int sx,
              int sy, const int16_t* __restrict__ plan, const uint8_t* __restrict__ wb, int plan_bw, int k, int n,
              const uint32_t* __restrict__ fallen, unsigned n_blocks)
{
    __shared__ __attribute__((aligned(16))) uint16_t res[kTH * kTW];
    __shared__ int off_ax[kTileBW * kTileBH], off_ay[kTileBW * kTileBH], off_bx[kTileBW * kTileBH], off_by[kTileBW * kTileBH];
    __shared__ int weight[kTileBW * kTileBH];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const long long plane = blockIdx.z;
    const int lbx = 4 - sx, lby = 4 - sy;                // log2 of the block's sides in this plane
    if (tid < kTileBW * kTileBH) {
        const int tx = tid % kTileBW, ty = tid / kTileBW;
        const int gx = (x0 >> lbx) + tx, gy = (y0 >> lby) + ty;          // x0 and y0 are multiples of a block's sides
        if (tx < (kTW >> lbx) && ty < (kTH >> lby) && (gx << lbx) < W && (gy << lby) < H) {
            const long long g = static_cast<long long>(gy) * plan_bw + gx;
            const bool all = fallen != nullptr && 2ULL * fallen[0] > n_blocks;
            const int16_t* p = plan + 4 * g;
            off_ax[tid] = all ? 0 : static_cast<int>(p[0]) >> sx;
            off_ay[tid] = all ? 0 : static_cast<int>(p[1]) >> sy;
            off_bx[tid] = all ? 0 : static_cast<int>(p[2]) >> sx;
            off_by[tid] = all ? 0 : static_cast<int>(p[3]) >> sy;
            weight[tid] = all ? (2 * k <= n ? 0 : n) : min(static_cast<int>(wb[g]), n);
        }
    }
    __syncthreads();
    const T* pa = a + plane * a_plane_stride;
    const T* pb = b + plane * b_plane_stride;
    constexpr int kRows = kThreads / kTW;
    const int tc = tid % kTW, tr = tid / kTW;
    const int x = x0 + tc;
    if (x < W) {
        for (int r = tr; r < kTH && y0 + r < H; r += kRows) {
            const int y = y0 + r;
            const int e = (r >> lby) * kTileBW + (tc >> lbx);
            const int w = weight[e];
            int sa = 0, sb = 0;
            if (w < n) sa = pa[static_cast<long long>(clampi(y + off_ay[e], 0, H - 1)) * a_row_stride + clampi(x + off_ax[e], 0, W - 1)];
            if (w > 0) sb = pb[static_cast<long long>(clampi(y + off_by[e], 0, H - 1)) * b_row_stride + clampi(x + off_bx[e], 0, W - 1)];
            res[r * kTW + tc] = static_cast<uint16_t>(static_cast<unsigned>((n - w) * sa + w * sb + (n >> 1)) / static_cast<unsigned>(n));
        }
    }
    __syncthreads();
    const int r = tid / (kTW / kOut), xo = (tid - r * (kTW / kOut)) * kOut;
    const int y = y0 + r, xs = x0 + xo;
    if (y >= H || xs >= W) return;
    const uint4 q = *reinterpret_cast<const uint4*>(res + r * kTW + xo);
    T* d = dst + plane * dst_plane_stride + static_cast<long long>(y) * dst_row_stride + xs;
    if (VEC_OUT && xs + kOut <= W) {
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
            if (xs + e < W) d[e] = static_cast<T>((w[e >> 1] >> (16 * (e & 1))) & 65535u);
        }
    }
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int blocks(int n, int b) { return (n + b - 1) / b; }

void check_samples(const std::string& w, int dtype, int bit_depth, bool depth_given, int H, int W)
{
    if (dtype != kSampleU8 && dtype != kSampleU16) throw std::invalid_argument(w + ": the sample type must be DCVC_SAMPLE_U8 or DCVC_SAMPLE_U16");
    if (depth_given && (dtype == kSampleU8 ? bit_depth != 8 : (bit_depth < 9 || bit_depth > 16))) {
        throw std::invalid_argument(w + ": bit_depth must be 8 (u8) or 9..16 (u16), got " + std::to_string(bit_depth));
    }
    if (H < 1 || W < 1 || H > kMotionMaxSide || W > kMotionMaxSide) {
        throw std::invalid_argument(w + ": sides must be in 1.." + std::to_string(kMotionMaxSide) + ", got " + std::to_string(W) + "x" + std::to_string(H));
    }
}

void check_phase(const std::string& w, int k, int n)
{
    if (n < kInterpMinN || n > kInterpMaxN) {
        throw std::invalid_argument(w + ": n must be in " + std::to_string(kInterpMinN) + ".." + std::to_string(kInterpMaxN) + ", got " + std::to_string(n));
    }
    if (k < 1 || k > n - 1) throw std::invalid_argument(w + ": k must be in 1..n-1 = 1.." + std::to_string(n - 1) + ", got " + std::to_string(k));
}

void check_grid(const std::string& w, const char* which, int bh, int bw, int need_bh, int need_bw)
{
    if (bh < need_bh || bw < need_bw || bh > kMotionMaxSide || bw > kMotionMaxSide) {
        throw std::invalid_argument(w + ": the " + which + " grid is " + std::to_string(bw) + "x" + std::to_string(bh) + ", the plane needs " +
                                    std::to_string(need_bw) + "x" + std::to_string(need_bh) + " (at most " + std::to_string(kMotionMaxSide) + " a side)");
    }
}

template <typename T>
void launch_select(const InterpSelectDesc& d, hipStream_t stream)
{
    hipLaunchKernelGGL(select_kernel<T>, dim3(blocks(d.W, kB), blocks(d.H, kB)), dim3(64), 0, stream, static_cast<const T*>(d.a),
                       static_cast<long long>(d.a_row_stride), static_cast<const T*>(d.b), static_cast<long long>(d.b_row_stride), d.H, d.W,
                       static_cast<const int16_t*>(d.mv), d.mv_bw, d.k, d.n, static_cast<unsigned>(d.limit) << (d.bit_depth - 8),
                       static_cast<int16_t*>(d.plan), static_cast<uint8_t*>(d.wb), d.plan_bw, static_cast<uint32_t*>(d.sad),
                       static_cast<uint32_t*>(d.fallen));
    hip_check(hipGetLastError(), "interp_select launch");
}

template <typename T>
void launch_planes(const InterpPlanesDesc& d, hipStream_t stream)
{
    const bool one = d.n_planes == 1;
    constexpr size_t al = kOut * sizeof(T);
    const bool vec_out = aligned(d.dst, al) && (d.dst_row_stride * sizeof(T)) % al == 0 && (one || (d.dst_plane_stride * sizeof(T)) % al == 0);
    const dim3 grid(blocks(d.W, kTW), blocks(d.H, kTH), d.n_planes);
    auto kern = vec_out ? interp_kernel<T, true> : interp_kernel<T, false>;
    hipLaunchKernelGGL(kern, grid, dim3(kThreads), 0, stream, static_cast<const T*>(d.a), static_cast<long long>(d.a_row_stride),
                       d.a_plane_stride, static_cast<const T*>(d.b), static_cast<long long>(d.b_row_stride), d.b_plane_stride,
                       static_cast<T*>(d.dst), static_cast<long long>(d.dst_row_stride), d.dst_plane_stride, d.H, d.W, d.sx, d.sy,
                       static_cast<const int16_t*>(d.plan), static_cast<const uint8_t*>(d.wb), d.plan_bw, d.k, d.n,
                       static_cast<const uint32_t*>(d.fallen), static_cast<unsigned>(d.n_blocks));
    hip_check(hipGetLastError(), "interp_planes launch");
}

}  // namespace

void interp_select_validate(const InterpSelectDesc& d)
{
    const std::string who = "interp_select";
    if (d.a == nullptr || d.b == nullptr || d.mv == nullptr || d.plan == nullptr || d.wb == nullptr) throw std::invalid_argument(who + ": null operand");
    check_samples(who, d.dtype, d.bit_depth, true, d.H, d.W);
    check_phase(who, d.k, d.n);
    if (d.limit < 0 || d.limit > kInterpMaxLimit) {
        throw std::invalid_argument(who + ": limit must be in 0.." + std::to_string(kInterpMaxLimit) + ", got " + std::to_string(d.limit));
    }
    check_grid(who, "mv", d.mv_bh, d.mv_bw, blocks(d.H, kB), blocks(d.W, kB));
    check_grid(who, "plan", d.plan_bh, d.plan_bw, blocks(d.H, kB), blocks(d.W, kB));
    if (d.a_row_stride < d.W || d.b_row_stride < d.W) throw std::invalid_argument(who + ": a row stride is below the width");
    const int es = d.dtype == kSampleU8 ? 1 : 2;
    if (!aligned(d.a, es) || !aligned(d.b, es)) throw std::invalid_argument(who + ": 16-bit planes must be 2-byte aligned");
    if (!aligned(d.mv, 2) || !aligned(d.plan, 2)) throw std::invalid_argument(who + ": mv and plan must be 2-byte aligned");
    if (!aligned(d.sad, 4) || !aligned(d.fallen, 4)) throw std::invalid_argument(who + ": sad and fallen must be 4-byte aligned");
}

void interp_select(const InterpSelectDesc& d, hipStream_t stream)
{
    interp_select_validate(d);
    if (d.dtype == kSampleU8) launch_select<uint8_t>(d, stream); else launch_select<uint16_t>(d, stream);
}

void interp_planes_validate(const InterpPlanesDesc& d)
{
    const std::string who = "interp_planes";
    if (d.a == nullptr || d.b == nullptr || d.dst == nullptr || d.plan == nullptr || d.wb == nullptr) throw std::invalid_argument(who + ": null operand");
    check_samples(who, d.dtype, 0, false, d.H, d.W);
    check_phase(who, d.k, d.n);
    if (d.sx < 0 || d.sx > 1 || d.sy < 0 || d.sy > 1) {
        throw std::invalid_argument(who + ": sx and sy must be 0 or 1, got " + std::to_string(d.sx) + ", " + std::to_string(d.sy));
    }
    if (d.n_planes < 1 || d.n_planes > 65535) throw std::invalid_argument(who + ": n_planes must be in 1..65535");
    check_grid(who, "plan", d.plan_bh, d.plan_bw, blocks(d.H, kB >> d.sy), blocks(d.W, kB >> d.sx));
    if (d.fallen != nullptr && d.n_blocks < 1) throw std::invalid_argument(who + ": n_blocks must be at least 1 with fallen, got " + std::to_string(d.n_blocks));
    if (d.a_row_stride < d.W || d.b_row_stride < d.W || d.dst_row_stride < d.W) throw std::invalid_argument(who + ": a row stride is below the width");
    const long long last = static_cast<long long>(d.H - 1);
    if (d.n_planes > 1 && (d.a_plane_stride < last * d.a_row_stride + d.W || d.b_plane_stride < last * d.b_row_stride + d.W ||
                           d.dst_plane_stride < last * d.dst_row_stride + d.W)) {
        throw std::invalid_argument(who + ": a plane stride is below the plane");
    }
    const int es = d.dtype == kSampleU8 ? 1 : 2;
    if (!aligned(d.a, es) || !aligned(d.b, es) || !aligned(d.dst, es)) throw std::invalid_argument(who + ": 16-bit planes must be 2-byte aligned");
    if (!aligned(d.plan, 2)) throw std::invalid_argument(who + ": plan must be 2-byte aligned");
    if (!aligned(d.fallen, 4)) throw std::invalid_argument(who + ": fallen must be 4-byte aligned");
    auto extent = [&](const void* p, long long row_stride, long long plane_stride, uintptr_t& lo, uintptr_t& hi) {
        lo = reinterpret_cast<uintptr_t>(p);
        hi = lo + static_cast<uintptr_t>((d.n_planes - 1) * plane_stride + (d.H - 1) * row_stride + d.W) * static_cast<uintptr_t>(es);
    };
    uintptr_t a0, a1, b0, b1, d0, d1;
    extent(d.a, d.a_row_stride, d.a_plane_stride, a0, a1);
    extent(d.b, d.b_row_stride, d.b_plane_stride, b0, b1);
    extent(d.dst, d.dst_row_stride, d.dst_plane_stride, d0, d1);
    if (a0 < d1 && d0 < a1) throw std::invalid_argument(who + ": dst overlaps a");
    if (b0 < d1 && d0 < b1) throw std::invalid_argument(who + ": dst overlaps b");
    const uintptr_t cells = static_cast<uintptr_t>(d.plan_bh) * d.plan_bw;
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(d.plan), p1 = p0 + cells * 4 * sizeof(int16_t);
    if (p0 < d1 && d0 < p1) throw std::invalid_argument(who + ": dst overlaps plan");
    const uintptr_t w0 = reinterpret_cast<uintptr_t>(d.wb), w1 = w0 + cells;
    if (w0 < d1 && d0 < w1) throw std::invalid_argument(who + ": dst overlaps wb");
}

void interp_planes(const InterpPlanesDesc& d, hipStream_t stream)
{
    interp_planes_validate(d);
    if (d.dtype == kSampleU8) launch_planes<uint8_t>(d, stream); else launch_planes<uint16_t>(d, stream);
}

}  // namespace dcvc
