// crop.hip - the two device pieces of black-bar cropping: crop_stats counts, per row and per column of a luma
// plane, the samples above a limit, and window_planes copies a window of a plane set into planes of another size, filling what
// the window shows beyond the source. Everything is an exact integer, so a numpy restatement (tests/crop_np.py) is held against
// both with ==. The decision over the counts is host code, dcvc_cropdet_* (dcvc_amd_rc.h).
//
// crop_stats. t = limit << (bit_depth - 8); rowcnt[r] = the number of x with Y[r][x] > t, colcnt[c] = the number of y with
// Y[y][c] > t; counts (device, uint32 [H + W]) = rowcnt, then colcnt.
//
// A workgroup of 256 threads takes a tile of kTileRows rows x kVecCols 16-byte vectors, field_match's shape; a thread walks
// down kRows rows of one vector column with a count per sample of its vector (its columns) and a count per row in registers.
// The 32 threads of a tile row are half a wave: the row counts go through shuffles inside the half, its first lane owns the
// row's LDS counter. The 8 threads of a vector column are two to a wave, 32 lanes apart: one shuffle adds the pair, then four
// waves add into the column's LDS counter. The workgroup issues one integer global atomic add per non-zero word. Integer adds
// commute, so the words are the same for every launch geometry and arrival order. A first, small launch zeroes the words: two
// launches, nothing allocated, no host wait.
//
// The bounds: a count is at most 16384, the largest side (static_assert below) - 15 bits in registers, LDS and the words.
//
// window_planes: dst[p][y][x] = src[p][y + oy][x + ox] where 0 <= y + oy < Hs and 0 <= x + ox < Ws, else fill[p]. ox, oy are
// signed: a crop (>= 0, the window inside the source), a pad (<= 0, the source inside the window) or any mixture. Planes ride in
// blockIdx.z, offsets are 64-bit, a thread writes one 16-byte vector of dst: a vector copy where the source address (offset
// included), dst and every stride are 16-byte aligned and the vector lies wholly inside both planes, a vector of fill where dst
// allows and the row lies outside the source, samples otherwise. Nothing is written past Wd. The fill values ride in the kernel
// arguments, kFillPlanes planes a launch.
#include "ops.h"

#include <algorithm>
#include <string>

namespace dcvc {

namespace {

constexpr int kThreads = 256;
constexpr int kVecCols = 32;                 // 16-byte vectors of a tile along x: half a wave
constexpr int kRows = 8;                     // rows a thread walks down
constexpr int kTileRows = kThreads / kVecCols * kRows;
constexpr int kMaxLimit = 255;
static_assert(kVecCols == 32 && kThreads % 64 == 0, "a tile row is one half of a wave, a vector column lanes l and l + 32 of every wave");
static_assert(kTileRows <= kThreads, "a thread per row word of the tile");
static_assert(kCropMaxSide <= 16384, "a count is at most 16384: a row holds W <= 16384 samples, a column H <= 16384");

template <typename T> struct Tile {
    static constexpr int V = 16 / static_cast<int>(sizeof(T));          // samples of a 16-byte vector
    static constexpr int cols = kVecCols * V;
};

// the samples above t among n (1..V) of a row from x on -> above[e] in {0, 1}, 0 past n; one 16-byte load where VEC says it is aligned
template <typename T, bool VEC>
__device__ __forceinline__ void load_above(const T* __restrict__ row, int n, unsigned t, unsigned (&above)[Tile<T>::V])
{
    constexpr int V = Tile<T>::V;
    if (VEC && n == V) {
        const uint4 v = *reinterpret_cast<const uint4*>(row);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
        if constexpr (sizeof(T) == 1) {
#pragma unroll
            for (int e = 0; e < V; ++e) above[e] = ((w[e >> 2] >> (8 * (e & 3))) & 255u) > t ? 1u : 0u;
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) above[e] = ((w[e >> 1] >> (16 * (e & 1))) & 65535u) > t ? 1u : 0u;
        }
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) above[e] = (e < n && static_cast<unsigned>(row[e]) > t) ? 1u : 0u;
    }
}

__global__ void crop_stats_zero_kernel(unsigned* __restrict__ counts, int n)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) counts[i] = 0u;
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(kThreads)
crop_stats_kernel(const T* __restrict__ luma, long long row_stride, int H, int W, unsigned t, unsigned* __restrict__ counts)
{
    using TL = Tile<T>;
    constexpr int V = TL::V;
    __shared__ unsigned rowc[kTileRows];             // the tile's row counters: one owner each
    __shared__ unsigned colc[TL::cols];              // the tile's column counters: the four waves add
    const int tid = threadIdx.x, tx = tid % kVecCols, ty = tid / kVecCols;
    for (int i = tid; i < TL::cols; i += kThreads) colc[i] = 0u;
    __syncthreads();
    const int x = blockIdx.x * TL::cols + tx * V, y0 = blockIdx.y * kTileRows + ty * kRows;
    const int n = min(V, W - x);                     // <= 0: the vector lies past the plane
    unsigned cc[V] = {}, rc[kRows] = {};
    if (n > 0) {
        const T* p = luma + static_cast<long long>(y0) * row_stride + x;
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            if (y0 + r < H) {
                unsigned above[V];
                load_above<T, VEC>(p + static_cast<long long>(r) * row_stride, n, t, above);
#pragma unroll
                for (int e = 0; e < V; ++e) { cc[e] += above[e]; rc[r] += above[e]; }
            }
        }
    }
    // rows: the 32 lanes of a half wave hold one tile row each of kRows
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        unsigned v = rc[r];
        for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (tx == 0) rowc[ty * kRows + r] = v;
    }
    // columns: lanes l and l + 32 of a wave hold the same vector column
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const unsigned v = cc[e] + __shfl_xor(cc[e], 32);
        if ((tid & 32) == 0 && v) atomicAdd(&colc[tx * V + e], v);
    }
    __syncthreads();
    if (tid < kTileRows) {
        const int y = blockIdx.y * kTileRows + tid;
        const unsigned v = rowc[tid];
        if (y < H && v) atomicAdd(counts + y, v);
    }
    for (int i = tid; i < TL::cols; i += kThreads) {
        const int c = blockIdx.x * TL::cols + i;
        const unsigned v = colc[i];
        if (c < W && v) atomicAdd(counts + H + c, v);
    }
}

constexpr int kWinX = 64, kWinY = 4;         // a workgroup writes kWinX vectors of kWinY rows
constexpr int kFillPlanes = 16;              // planes a launch: their fill values are kernel arguments
static_assert(kWinX * kWinY == kThreads, "a vector per thread");
struct Fills { int v[kFillPlanes]; };

// MODE 0: samples only; 1: dst takes 16-byte stores (the fill); 2: the source does too (the copy)
template <typename T, int MODE>
__global__ void __launch_bounds__(kThreads)
window_planes_kernel(const T* __restrict__ src, long long src_row_stride, long long src_plane_stride, int Hs, int Ws, T* __restrict__ dst,
                     long long dst_row_stride, long long dst_plane_stride, int Hd, int Wd, int ox, int oy, Fills fills)
{
    constexpr int V = Tile<T>::V;
    const int x = (blockIdx.x * kWinX + threadIdx.x % kWinX) * V, y = blockIdx.y * kWinY + threadIdx.x / kWinX;
    if (x >= Wd || y >= Hd) return;
    const long long plane = blockIdx.z;
    const unsigned fill = static_cast<unsigned>(fills.v[blockIdx.z]);
    const int ys = y + oy, xs = x + ox;
    const bool row_in = ys >= 0 && ys < Hs;
    T* d = dst + plane * dst_plane_stride + static_cast<long long>(y) * dst_row_stride + x;
    // the row of the source this dst row shows; not formed (and never read) for a row outside it
    const T* s = row_in ? src + plane * src_plane_stride + static_cast<long long>(ys) * src_row_stride : nullptr;
    const bool whole = x + V <= Wd;
    if (MODE == 2 && whole && row_in && xs >= 0 && xs + V <= Ws) {
        *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s + xs);
    } else if (MODE >= 1 && whole && (!row_in || xs + V <= 0 || xs >= Ws)) {
        const unsigned w = sizeof(T) == 1 ? fill * 0x01010101u : fill * 0x00010001u;
        *reinterpret_cast<uint4*>(d) = make_uint4(w, w, w, w);
    } else {
        const int n = min(V, Wd - x);
        for (int e = 0; e < n; ++e) {
            const int xe = xs + e;
            d[e] = (row_in && xe >= 0 && xe < Ws) ? s[xe] : static_cast<T>(fill);
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

// what both entries refuse alike; `who` names the kernel in the message
int sample_bytes(const char* who, int dtype)
{
    if (dtype != kSampleU8 && dtype != kSampleU16) {
        throw std::invalid_argument(std::string(who) + ": the sample type must be DCVC_SAMPLE_U8 or DCVC_SAMPLE_U16");
    }
    return dtype == kSampleU8 ? 1 : 2;
}

void check_side(const char* who, const char* what, int h, int w)
{
    if (h < 1 || h > kCropMaxSide || w < 1 || w > kCropMaxSide) {
        throw std::invalid_argument(std::string(who) + ": " + what + " must be in 1.." + std::to_string(kCropMaxSide) + " a side, got " +
                                    std::to_string(w) + "x" + std::to_string(h));
    }
}

template <typename T>
void launch_stats(const CropStatsDesc& d, hipStream_t stream)
{
    const T* luma = static_cast<const T*>(d.luma);
    unsigned* counts = static_cast<unsigned*>(d.counts);
    const bool vec = aligned(luma, 16) && (static_cast<long long>(d.row_stride) * sizeof(T)) % 16 == 0;
    const int words = d.H + d.W;
    hipLaunchKernelGGL(crop_stats_zero_kernel, dim3((words + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, counts, words);
    hip_check(hipGetLastError(), "crop_stats zero launch");
    const dim3 grid((d.W + Tile<T>::cols - 1) / Tile<T>::cols, (d.H + kTileRows - 1) / kTileRows);
    auto k = vec ? crop_stats_kernel<T, true> : crop_stats_kernel<T, false>;
    hipLaunchKernelGGL(k, grid, dim3(kThreads), 0, stream, luma, static_cast<long long>(d.row_stride), d.H, d.W,
                       static_cast<unsigned>(d.limit) << (d.bit_depth - 8), counts);
    hip_check(hipGetLastError(), "crop_stats launch");
}

template <typename T>
void launch_window(const WindowPlanesDesc& d, hipStream_t stream)
{
    const bool one = d.n_planes == 1;
    auto fits = [&](const void* p, long long row_stride, long long plane_stride) {
        return aligned(p, 16) && (row_stride * sizeof(T)) % 16 == 0 && (one || (plane_stride * sizeof(T)) % 16 == 0);
    };
    const T* src = static_cast<const T*>(d.src);
    T* dst = static_cast<T*>(d.dst);
    // the source vector of dst vector (y, x) starts (y + oy) rows and x + ox samples in: aligned when the offset's bytes are
    const long long off = (static_cast<long long>(d.oy) * d.src_row_stride + d.ox) * static_cast<long long>(sizeof(T));
    const bool dvec = fits(dst, d.dst_row_stride, d.dst_plane_stride);
    const bool svec = dvec && fits(src, d.src_row_stride, d.src_plane_stride) && off % 16 == 0;
    constexpr int V = Tile<T>::V;
    auto k = svec ? window_planes_kernel<T, 2> : dvec ? window_planes_kernel<T, 1> : window_planes_kernel<T, 0>;
    for (int p0 = 0; p0 < d.n_planes; p0 += kFillPlanes) {
        const int np = std::min(kFillPlanes, d.n_planes - p0);
        Fills fills = {};
        for (int i = 0; i < np; ++i) fills.v[i] = d.fill[p0 + i];
        const dim3 grid((d.Wd + kWinX * V - 1) / (kWinX * V), (d.Hd + kWinY - 1) / kWinY, np);
        hipLaunchKernelGGL(k, grid, dim3(kThreads), 0, stream, src + p0 * d.src_plane_stride, static_cast<long long>(d.src_row_stride),
                           d.src_plane_stride, d.Hs, d.Ws, dst + p0 * d.dst_plane_stride, static_cast<long long>(d.dst_row_stride),
                           d.dst_plane_stride, d.Hd, d.Wd, d.ox, d.oy, fills);
        hip_check(hipGetLastError(), "window_planes launch");
    }
}

}  // namespace

void crop_stats_validate(const CropStatsDesc& d)
{
    if (d.luma == nullptr || d.counts == nullptr) throw std::invalid_argument("crop_stats: null operand");
    const int es = sample_bytes("crop_stats", d.dtype);
    if (es == 1 ? d.bit_depth != 8 : (d.bit_depth < 9 || d.bit_depth > 16)) {
        throw std::invalid_argument("crop_stats: bit_depth must be 8 (u8) or 9..16 (u16), got " + std::to_string(d.bit_depth));
    }
    check_side("crop_stats", "the plane", d.H, d.W);
    if (d.limit < 0 || d.limit > kMaxLimit) throw std::invalid_argument("crop_stats: limit must be in 0..255, got " + std::to_string(d.limit));
    if (d.row_stride < d.W) throw std::invalid_argument("crop_stats: the row stride is below the width");
    if (!aligned(d.luma, es)) throw std::invalid_argument("crop_stats: a 16-bit plane must be 2-byte aligned");
    if (!aligned(d.counts, 4)) throw std::invalid_argument("crop_stats: counts must be 4-byte aligned");
}

void crop_stats(const CropStatsDesc& d, hipStream_t stream)
{
    crop_stats_validate(d);
    if (d.dtype == kSampleU8) launch_stats<uint8_t>(d, stream); else launch_stats<uint16_t>(d, stream);
}

void window_planes_validate(const WindowPlanesDesc& d)
{
    if (d.src == nullptr || d.dst == nullptr || d.fill == nullptr) throw std::invalid_argument("window_planes: null operand");
    const int es = sample_bytes("window_planes", d.dtype);
    check_side("window_planes", "the source", d.Hs, d.Ws);
    check_side("window_planes", "the window", d.Hd, d.Wd);
    if (d.n_planes < 1 || d.n_planes > 65535) throw std::invalid_argument("window_planes: n_planes must be in 1..65535");
    if (d.ox < -kCropMaxSide || d.ox > kCropMaxSide || d.oy < -kCropMaxSide || d.oy > kCropMaxSide) {
        throw std::invalid_argument("window_planes: the offsets must be in -" + std::to_string(kCropMaxSide) + ".." + std::to_string(kCropMaxSide) +
                                    ", got " + std::to_string(d.ox) + ", " + std::to_string(d.oy));
    }
    const int max_val = es == 1 ? 255 : 65535;
    for (int p = 0; p < d.n_planes; ++p) {
        if (d.fill[p] < 0 || d.fill[p] > max_val) {
            throw std::invalid_argument("window_planes: fill value " + std::to_string(d.fill[p]) + " of plane " + std::to_string(p) +
                                        " is outside 0.." + std::to_string(max_val));
        }
    }
    if (d.src_row_stride < d.Ws || d.dst_row_stride < d.Wd) throw std::invalid_argument("window_planes: a row stride is below the width");
    if (d.n_planes > 1 && (d.src_plane_stride < static_cast<long long>(d.Hs - 1) * d.src_row_stride + d.Ws ||
                           d.dst_plane_stride < static_cast<long long>(d.Hd - 1) * d.dst_row_stride + d.Wd)) {
        throw std::invalid_argument("window_planes: a plane stride is below the plane");
    }
    if (!aligned(d.src, es) || !aligned(d.dst, es)) throw std::invalid_argument("window_planes: 16-bit planes must be 2-byte aligned");
    uintptr_t s0, s1, d0, d1;
    extent(d.src, es, d.n_planes, d.Hs, d.Ws, d.src_row_stride, d.src_plane_stride, s0, s1);
    extent(d.dst, es, d.n_planes, d.Hd, d.Wd, d.dst_row_stride, d.dst_plane_stride, d0, d1);
    if (s0 < d1 && d0 < s1) throw std::invalid_argument("window_planes: dst overlaps src");
}

void window_planes(const WindowPlanesDesc& d, hipStream_t stream)
{
    window_planes_validate(d);
    if (d.dtype == kSampleU8) launch_window<uint8_t>(d, stream); else launch_window<uint16_t>(d, stream);
}

}  // namespace dcvc
