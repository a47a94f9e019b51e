// motion.hip - a block motion search between two luma planes and the motion compensation of planes through its vectors
// (DESIGN.md 31). Everything is defined exactly, in signed 32-bit integers, so a numpy restatement (tests/motion_np.py) can be
// held against both kernels with ==.
//
// sh = bit_depth - 8, L = lambda << sh. Blocks are 16 x 16 luma samples, Bh = ceil(H / 16), Bw = ceil(W / 16).
//   half resolution: H1 = ceil(H / 2), W1 = ceil(W / 2),
//                    a1[y][x] = (a[2y][2x] + a[2y][2x+1] + a[2y+1][2x] + a[2y+1][2x+1] + 2) >> 2, indexes clamped to the plane.
//   block SAD:       over the block's samples that lie inside cur (a partial block at the right or bottom edge sums fewer);
//                    the reference index (y + dy, x + dx) is clamped to the plane.
//   order:           the smallest tuple (cost, |dx| + |dy|, dy, dx) wins.
//   level 1:         block (by, bx) is the 8 x 8 block of the half-resolution planes; every dx, dy in -R..R is a candidate,
//                    cost = SAD + L (|dx| + |dy|); the winner is (dx1, dy1).
//   level 0:         full resolution, the 16 x 16 block; the candidates are (2 dx1 + ex, 2 dy1 + ey), ex, ey in -1..1, and
//                    (0, 0); cost = SAD + 4 L (|dx| + |dy|). The winner goes to mv, its SAD (without the penalty) to sad.
//   compensation:    a plane subsampled by (sx, sy) against that luma plane: the block of sample (y, x) is
//                    (y / (16 >> sy), x / (16 >> sx)), dxc = dx >> sx, dyc = dy >> sy (arithmetic shifts: a floor),
//                    dst[y][x] = prev[clamp(y + dyc)][clamp(x + dxc)]. Any int16 vector is safe: the clamp bounds every read.
//
// Bounds: |mv| <= 2 R + 1 <= 31; the largest cost is 256 * 65535 + 4 * (255 << 8) * 62 < 2^31 (static_assert below). A candidate
// is ordered by one 64-bit key, cost << 20 | (|dx| + |dy|) << 14 | (dy + 64) << 7 | (dx + 64), whose order is the tuple's.
//
// motion_search is two launches. The first writes the two half-resolution planes, 16-bit words, into the caller's workspace.
// The second runs one wave per block: it stages the block's 8 x 8 half-resolution samples and its (8 + 2 R)^2 reference window
// in LDS, the clamp applied while staging; each lane owns candidates, (2 R + 1)^2 <= 961 of them in rounds of 64, and sums the
// block's 64 differences from LDS (the block's sample is one address for the wave, a broadcast; the window's addresses are
// consecutive along dx); one cross-lane minimum over the key gives (dx1, dy1) to
// every lane. Then the 16 x 16 block, the 18 x 18 window around (2 dx1, 2 dy1) and the co-located block are staged, lanes run
// over samples (4 each), and a wave sum per candidate gives its SAD to every lane; lane 0 stores the winner and counts it in
// `moved` (one integer atomic) if it is not (0, 0).
//
// motion_compensate_planes is one launch: planes of one size ride in blockIdx.z, plane offsets are 64-bit. A workgroup of 256
// threads makes a tile of kTW x kTH outputs, threads along x while they fetch (the reads of a block are consecutive), the
// results pass through LDS so that a thread stores 8 consecutive samples as one 8- or 16-byte word (VEC_OUT) where dst's base
// and strides allow, as denoise.hip does. Nothing is written past W.
#include "ops.h"

#include <string>

namespace dcvc {

namespace {

constexpr int kB = kMotionBlock;             // luma samples a block side
constexpr int kB1 = kB / 2;                  // ... at half resolution
constexpr int kMaxWin = kB1 + 2 * kMotionMaxRange;       // the level-1 window's side at the largest range
constexpr int kWin0 = kB + 2;                // the level-0 window's side
constexpr long long kMaxCost = 256LL * 65535 + 4LL * (static_cast<long long>(kMotionMaxLambda) << 8) * (2 * (2 * kMotionMaxRange + 1));
static_assert(kMaxCost < (1LL << 31), "a cost must fit the 32-bit accumulator");
static_assert(2 * kMotionMaxRange + 1 < 64 && 2 * (2 * kMotionMaxRange + 1) < 64, "a component must fit 7 bits with its offset, the length 6 bits");

constexpr int kHalfTX = 64, kHalfTY = 4;     // the half-resolution launch: 256 threads, 64 x 4 outputs

constexpr int kThreads = 256;                // the compensation launch
constexpr int kTW = 128;
constexpr int kTH = 16;
constexpr int kOut = 8;
static_assert(kTW * kTH == kThreads * kOut, "one store of kOut samples per thread");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// z = 0: cur, z = 1: ref -> half [z][H1][W1]
template <typename T>
__global__ void __launch_bounds__(kHalfTX * kHalfTY)
half_kernel(const T* __restrict__ cur, long long cur_row_stride, const T* __restrict__ ref, long long ref_row_stride, int H, int W,
            int H1, int W1, uint16_t* __restrict__ half)
{
    const int x = blockIdx.x * kHalfTX + (threadIdx.x % kHalfTX), y = blockIdx.y * kHalfTY + (threadIdx.x / kHalfTX);
    if (x >= W1 || y >= H1) return;
    const T* a = blockIdx.z == 0 ? cur : ref;
    const long long rs = blockIdx.z == 0 ? cur_row_stride : ref_row_stride;
    const int xa = 2 * x, xb = min(2 * x + 1, W - 1), ya = 2 * y, yb = min(2 * y + 1, H - 1);
    const T* ra = a + ya * rs;
    const T* rb = a + yb * rs;
    const int s = static_cast<int>(ra[xa]) + static_cast<int>(ra[xb]) + static_cast<int>(rb[xa]) + static_cast<int>(rb[xb]);
    half[(static_cast<long long>(blockIdx.z) * H1 + y) * W1 + x] = static_cast<uint16_t>((s + 2) >> 2);
}

__device__ __forceinline__ unsigned long long pack_key(int cost, int dx, int dy)
{
    return (static_cast<unsigned long long>(cost) << 20) | (static_cast<unsigned long long>(abs(dx) + abs(dy)) << 14) |
           (static_cast<unsigned long long>(dy + 64) << 7) | static_cast<unsigned long long>(dx + 64);
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long k)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off, 64);
        k = o < k ? o : k;
    }
    return k;
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// one wave per block (by, bx) = (blockIdx.y, blockIdx.x)
template <typename T>
__global__ void __launch_bounds__(64)
search_kernel(const uint16_t* __restrict__ half, int H1, int W1, const T* __restrict__ cur, long long cur_row_stride,
              const T* __restrict__ ref, long long ref_row_stride, int H, int W, int R, int L, int16_t* __restrict__ mv,
              uint32_t* __restrict__ sad_out, uint32_t* __restrict__ moved, int mv_bw)
{
    __shared__ uint16_t c1s[kB1 * kB1];              // the block at half resolution
    __shared__ uint16_t w1s[kMaxWin * kMaxWin];      // its reference window, pitch 8 + 2 R
    __shared__ uint16_t c0s[kB * kB];                // the block at full resolution
    __shared__ uint16_t z0s[kB * kB];                // the co-located reference block
    __shared__ uint16_t w0s[kWin0 * kWin0];          // the reference window around (2 dx1, 2 dy1)
    const int lane = threadIdx.x;
    const int bx = blockIdx.x, by = blockIdx.y;

    // ---- level 1
    const uint16_t* c1 = half;
    const uint16_t* r1 = half + static_cast<long long>(H1) * W1;
    const int x1 = bx * kB1, y1 = by * kB1;
    const int bw1 = min(kB1, W1 - x1), bh1 = min(kB1, H1 - y1);      // >= 1: ceil(ceil(H / 2) / 8) == ceil(H / 16)
    const int n = kB1 + 2 * R, nc = 2 * R + 1;
    c1s[lane] = c1[static_cast<long long>(min(y1 + (lane >> 3), H1 - 1)) * W1 + min(x1 + (lane & 7), W1 - 1)];
    for (int i = lane; i < n * n; i += 64) {
        const int r = i / n, c = i - r * n;
        w1s[i] = r1[static_cast<long long>(clampi(y1 - R + r, 0, H1 - 1)) * W1 + clampi(x1 - R + c, 0, W1 - 1)];
    }
    __syncthreads();
    unsigned long long best = ~0ULL;
    const bool whole1 = bw1 == kB1 && bh1 == kB1;
    for (int c = lane; c < nc * nc; c += 64) {
        const int dyi = c / nc, dxi = c - dyi * nc;
        const uint16_t* w = w1s + dyi * n + dxi;
        unsigned s = 0;
        if (whole1) {
#pragma unroll
            for (int r = 0; r < kB1; ++r) {
#pragma unroll
                for (int q = 0; q < kB1; ++q) s = __usad(c1s[r * kB1 + q], w[r * n + q], s);
            }
        } else {
            for (int r = 0; r < bh1; ++r) {
                for (int q = 0; q < bw1; ++q) s = __usad(c1s[r * kB1 + q], w[r * n + q], s);
            }
        }
        const int dx = dxi - R, dy = dyi - R;
        const unsigned long long k = pack_key(static_cast<int>(s) + L * (abs(dx) + abs(dy)), dx, dy);
        best = k < best ? k : best;
    }
    best = wave_min(best);
    const int dx1 = static_cast<int>(best & 127) - 64, dy1 = static_cast<int>((best >> 7) & 127) - 64;

    // ---- level 0
    const int x0 = bx * kB, y0 = by * kB;
    const int bw0 = min(kB, W - x0), bh0 = min(kB, H - y0);
    for (int i = lane; i < kB * kB; i += 64) {
        const int r = i / kB, c = i % kB;
        const long long yy = min(y0 + r, H - 1);
        const int xx = min(x0 + c, W - 1);
        c0s[i] = static_cast<uint16_t>(cur[yy * cur_row_stride + xx]);
        z0s[i] = static_cast<uint16_t>(ref[yy * ref_row_stride + xx]);
    }
    for (int i = lane; i < kWin0 * kWin0; i += 64) {
        const int r = i / kWin0, c = i - r * kWin0;
        const long long yy = clampi(y0 + 2 * dy1 - 1 + r, 0, H - 1);
        w0s[i] = static_cast<uint16_t>(ref[yy * ref_row_stride + clampi(x0 + 2 * dx1 - 1 + c, 0, W - 1)]);
    }
    __syncthreads();
    // the samples of this lane: i = lane + 64 k, row i / 16, column i % 16
    int cs[4];
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = lane + 64 * k;
        cs[k] = c0s[i];
        in[k] = (i / kB) < bh0 && (i % kB) < bw0;
    }
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += in[k] ? __usad(cs[k], z0s[lane + 64 * k], 0u) : 0u;
    int best_sad = wave_sum(static_cast<int>(s));
    best = pack_key(best_sad, 0, 0);
    for (int e = 0; e < 9; ++e) {
        const int ey = e / 3, ex = e - ey * 3;           // the offsets + 1: the window starts at (-1, -1)
        s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = lane + 64 * k;
            s += in[k] ? __usad(cs[k], w0s[((i / kB) + ey) * kWin0 + (i % kB) + ex], 0u) : 0u;
        }
        const int total = wave_sum(static_cast<int>(s));
        const int dx = 2 * dx1 + ex - 1, dy = 2 * dy1 + ey - 1;
        const unsigned long long k = pack_key(total + 4 * L * (abs(dx) + abs(dy)), dx, dy);
        if (k < best) { best = k; best_sad = total; }
    }
    if (lane == 0) {
        const long long b = static_cast<long long>(by) * mv_bw + bx;
        mv[2 * b] = static_cast<int16_t>(static_cast<int>(best & 127) - 64);
        mv[2 * b + 1] = static_cast<int16_t>(static_cast<int>((best >> 7) & 127) - 64);
        if (sad_out) sad_out[b] = static_cast<uint32_t>(best_sad);
        if (moved && (best & 0x3fff) != ((64u << 7) | 64u)) atomicAdd(moved, 1u);
    }
}

template <typename T, bool VEC_OUT>
__global__ void __launch_bounds__(kThreads)
compensate_kernel(const T* __restrict__ prev, long long prev_row_stride, long long prev_plane_stride, T* __restrict__ dst,
                  long long dst_row_stride, long long dst_plane_stride, int H, int W, int sx, int sy, const int16_t* __restrict__ mv,
                  int mv_bw)
{
    __shared__ __attribute__((aligned(16))) uint16_t res[kTH * kTW];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const long long plane = blockIdx.z;
    const T* p = prev + plane * prev_plane_stride;
    constexpr int kRows = kThreads / kTW;
    const int tc = tid % kTW, tr = tid / kTW;
    const int x = x0 + tc;
    const int lbx = 4 - sx, lby = 4 - sy;                // log2 of the block's sides in this plane
    if (x < W) {
        for (int r = tr; r < kTH && y0 + r < H; r += kRows) {
            const int y = y0 + r;
            const int16_t* v = mv + 2 * (static_cast<long long>(y >> lby) * mv_bw + (x >> lbx));
            const int dxc = static_cast<int>(v[0]) >> sx, dyc = static_cast<int>(v[1]) >> sy;
            res[r * kTW + tc] = static_cast<uint16_t>(p[static_cast<long long>(clampi(y + dyc, 0, H - 1)) * prev_row_stride + clampi(x + dxc, 0, W - 1)]);
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

void check_samples(const char* who, int dtype, int bit_depth, bool depth_given, int H, int W)
{
    const std::string w(who);
    if (dtype != kSampleU8 && dtype != kSampleU16) throw std::invalid_argument(w + ": the sample type must be DCVC_SAMPLE_U8 or DCVC_SAMPLE_U16");
    if (depth_given && (dtype == kSampleU8 ? bit_depth != 8 : (bit_depth < 9 || bit_depth > 16))) {
        throw std::invalid_argument(w + ": bit_depth must be 8 (u8) or 9..16 (u16), got " + std::to_string(bit_depth));
    }
    if (H < 1 || W < 1 || H > kMotionMaxSide || W > kMotionMaxSide) {
        throw std::invalid_argument(w + ": sides must be in 1.." + std::to_string(kMotionMaxSide) + ", got " + std::to_string(W) + "x" + std::to_string(H));
    }
}

void check_grid(const char* who, int mv_bh, int mv_bw, int need_bh, int need_bw)
{
    if (mv_bh < need_bh || mv_bw < need_bw || mv_bh > kMotionMaxSide || mv_bw > kMotionMaxSide) {
        throw std::invalid_argument(std::string(who) + ": the mv grid is " + std::to_string(mv_bw) + "x" + std::to_string(mv_bh) + ", the plane needs " +
                                    std::to_string(need_bw) + "x" + std::to_string(need_bh) + " (at most " + std::to_string(kMotionMaxSide) + " a side)");
    }
}

template <typename T>
void launch_search(const MotionSearchDesc& d, hipStream_t stream)
{
    const T* cur = static_cast<const T*>(d.cur);
    const T* ref = static_cast<const T*>(d.ref);
    uint16_t* half = static_cast<uint16_t*>(d.workspace);
    const int H1 = (d.H + 1) / 2, W1 = (d.W + 1) / 2;
    hipLaunchKernelGGL(half_kernel<T>, dim3(blocks(W1, kHalfTX), blocks(H1, kHalfTY), 2), dim3(kHalfTX * kHalfTY), 0, stream, cur,
                       static_cast<long long>(d.cur_row_stride), ref, static_cast<long long>(d.ref_row_stride), d.H, d.W, H1, W1, half);
    hip_check(hipGetLastError(), "motion_search half-resolution launch");
    hipLaunchKernelGGL(search_kernel<T>, dim3(blocks(d.W, kB), blocks(d.H, kB)), dim3(64), 0, stream, half, H1, W1, cur,
                       static_cast<long long>(d.cur_row_stride), ref, static_cast<long long>(d.ref_row_stride), d.H, d.W, d.range,
                       d.lambda << (d.bit_depth - 8), static_cast<int16_t*>(d.mv), static_cast<uint32_t*>(d.sad), static_cast<uint32_t*>(d.moved), d.mv_bw);
    hip_check(hipGetLastError(), "motion_search launch");
}

template <typename T>
void launch_compensate(const MotionCompensateDesc& d, hipStream_t stream)
{
    const bool one = d.n_planes == 1;
    constexpr size_t a = kOut * sizeof(T);
    const bool vec_out = aligned(d.dst, a) && (d.dst_row_stride * sizeof(T)) % a == 0 && (one || (d.dst_plane_stride * sizeof(T)) % a == 0);
    const dim3 grid(blocks(d.W, kTW), blocks(d.H, kTH), d.n_planes);
    auto k = vec_out ? compensate_kernel<T, true> : compensate_kernel<T, false>;
    hipLaunchKernelGGL(k, grid, dim3(kThreads), 0, stream, static_cast<const T*>(d.prev), static_cast<long long>(d.prev_row_stride),
                       d.prev_plane_stride, static_cast<T*>(d.dst), static_cast<long long>(d.dst_row_stride), d.dst_plane_stride, d.H, d.W,
                       d.sx, d.sy, static_cast<const int16_t*>(d.mv), d.mv_bw);
    hip_check(hipGetLastError(), "motion_compensate launch");
}

}  // namespace

size_t motion_search_workspace_bytes(int H, int W)
{
    return 2 * static_cast<size_t>((H + 1) / 2) * static_cast<size_t>((W + 1) / 2) * sizeof(uint16_t);
}

void motion_search_validate(const MotionSearchDesc& d)
{
    const char* who = "motion_search";
    if (d.cur == nullptr || d.ref == nullptr || d.mv == nullptr || d.workspace == nullptr) throw std::invalid_argument("motion_search: null operand");
    check_samples(who, d.dtype, d.bit_depth, true, d.H, d.W);
    if (d.range < 0 || d.range > kMotionMaxRange) {
        throw std::invalid_argument("motion_search: the range must be in 0.." + std::to_string(kMotionMaxRange) + ", got " + std::to_string(d.range));
    }
    if (d.lambda < 0 || d.lambda > kMotionMaxLambda) {
        throw std::invalid_argument("motion_search: lambda must be in 0.." + std::to_string(kMotionMaxLambda) + ", got " + std::to_string(d.lambda));
    }
    check_grid(who, d.mv_bh, d.mv_bw, blocks(d.H, kB), blocks(d.W, kB));
    if (d.cur_row_stride < d.W || d.ref_row_stride < d.W) throw std::invalid_argument("motion_search: a row stride is below the width");
    const int es = d.dtype == kSampleU8 ? 1 : 2;
    if (!aligned(d.cur, es) || !aligned(d.ref, es)) throw std::invalid_argument("motion_search: 16-bit planes must be 2-byte aligned");
    if (!aligned(d.mv, 2)) throw std::invalid_argument("motion_search: mv must be 2-byte aligned");
    if (!aligned(d.sad, 4) || !aligned(d.moved, 4)) throw std::invalid_argument("motion_search: sad and moved must be 4-byte aligned");
    if (!aligned(d.workspace, 2) || d.workspace_bytes < 0 ||
        static_cast<unsigned long long>(d.workspace_bytes) < motion_search_workspace_bytes(d.H, d.W)) {
        throw std::invalid_argument("motion_search: workspace misaligned or smaller than dcvc_motion_search_workspace_bytes");
    }
}

void motion_search(const MotionSearchDesc& d, hipStream_t stream)
{
    motion_search_validate(d);
    if (d.dtype == kSampleU8) launch_search<uint8_t>(d, stream); else launch_search<uint16_t>(d, stream);
}

void motion_compensate_validate(const MotionCompensateDesc& d)
{
    const char* who = "motion_compensate";
    if (d.prev == nullptr || d.dst == nullptr || d.mv == nullptr) throw std::invalid_argument("motion_compensate: null operand");
    check_samples(who, d.dtype, 0, false, d.H, d.W);
    if (d.sx < 0 || d.sx > 1 || d.sy < 0 || d.sy > 1) {
        throw std::invalid_argument("motion_compensate: sx and sy must be 0 or 1, got " + std::to_string(d.sx) + ", " + std::to_string(d.sy));
    }
    if (d.n_planes < 1 || d.n_planes > 65535) throw std::invalid_argument("motion_compensate: n_planes must be in 1..65535");
    check_grid(who, d.mv_bh, d.mv_bw, blocks(d.H, kB >> d.sy), blocks(d.W, kB >> d.sx));
    if (d.prev_row_stride < d.W || d.dst_row_stride < d.W) throw std::invalid_argument("motion_compensate: a row stride is below the width");
    const long long plane = static_cast<long long>(d.H - 1);
    if (d.n_planes > 1 && (d.prev_plane_stride < plane * d.prev_row_stride + d.W || d.dst_plane_stride < plane * d.dst_row_stride + d.W)) {
        throw std::invalid_argument("motion_compensate: a plane stride is below the plane");
    }
    const int es = d.dtype == kSampleU8 ? 1 : 2;
    if (!aligned(d.prev, es) || !aligned(d.dst, es)) throw std::invalid_argument("motion_compensate: 16-bit planes must be 2-byte aligned");
    if (!aligned(d.mv, 2)) throw std::invalid_argument("motion_compensate: mv must be 2-byte aligned");
    auto extent = [&](const void* p, long long row_stride, long long plane_stride, uintptr_t& lo, uintptr_t& hi) {
        lo = reinterpret_cast<uintptr_t>(p);
        hi = lo + static_cast<uintptr_t>((d.n_planes - 1) * plane_stride + (d.H - 1) * row_stride + d.W) * static_cast<uintptr_t>(es);
    };
    uintptr_t p0, p1, d0, d1;
    extent(d.prev, d.prev_row_stride, d.prev_plane_stride, p0, p1);
    extent(d.dst, d.dst_row_stride, d.dst_plane_stride, d0, d1);
    if (p0 < d1 && d0 < p1) throw std::invalid_argument("motion_compensate: dst overlaps prev");
    const uintptr_t m0 = reinterpret_cast<uintptr_t>(d.mv), m1 = m0 + static_cast<uintptr_t>(d.mv_bh) * d.mv_bw * 2 * sizeof(int16_t);
    if (m0 < d1 && d0 < m1) throw std::invalid_argument("motion_compensate: dst overlaps mv");
}

void motion_compensate_planes(const MotionCompensateDesc& d, hipStream_t stream)
{
    motion_compensate_validate(d);
    if (d.dtype == kSampleU8) launch_compensate<uint8_t>(d, stream); else launch_compensate<uint16_t>(d, stream);
}

}  // namespace dcvc
