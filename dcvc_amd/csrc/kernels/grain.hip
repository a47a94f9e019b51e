// grain.hip - the two device pieces of film grain: grain_apply puts synthetic grain onto the planes of a decoded
// picture, grain_stats measures what the denoising prefilter (denoise.hip) took out of a source picture. Everything is an exact
// integer, so a numpy restatement (tests/grain_np.py) is held against both with ==.
//
// sh = bit_depth - 8, max_val = 2^bit_depth - 1; u32 arithmetic wraps; shifts of signed values are arithmetic.
//
// Collocated luma of the sample (y, x) of a plane subsampled by (sx, sy) in {0, 1} against a luma plane Yl [Hl][Wl], indexes
// clamped into the luma plane:
//   sx == 1: L = (Yl[y << sy][x << sx] + Yl[y << sy][(x << sx) + 1] + 1) >> 1;   sx == 0: L = Yl[y << sy][x]
//   i = min(L >> sh, 255) (the min binds only for samples above max_val, which no picture of that depth holds)
//
// grain_apply. Plane p (0, 1, 2 = Y, U, V) of output picture `pic` is cut into blocks of 32 x 32 samples; block (by, bx) takes
//   h = seed*0x9E3779B1 + pic*0x85EBCA77 + p*0xC2B2AE3D + by*0x27D4EB2F + bx*0x165667B1
//   h ^= h >> 15; h *= 0x2C1B3C6D; h ^= h >> 12; h *= 0x297A2D39; h ^= h >> 15; ox = h & 63; oy = (h >> 8) & 63
//   t = T_p[(oy + (y & 31)) & 63][(ox + (x & 31)) & 63]                      T_p: the plane's 64 x 64 int16 template, |t| <= 1023
//   k = i >> 5, fr = i & 31, v = (lut[k] (32 - fr) + lut[k + 1] fr + 16) >> 5    lut: nine entries 0..255, sixteenths of a code value
//   n = (t v + (1 << (9 - sh))) >> (10 - sh)
//   out = clamp(rec + n, 0, max_val)
// |t v| <= 1023 * 255 < 2^18 and |n| < 2^16 at sh = 8: everything fits 32 bits with room.
// One launch: planes of one size ride in blockIdx.z, plane offsets are 64-bit. A workgroup of 256 threads stages its plane's
// template (8 KB) and table in LDS once and covers a tile of kTW x kTH samples - a whole number of blocks - in kTW * kTH / 8 /
// 256 passes; a thread takes 8 consecutive samples of a row (they lie in one block) with one 8-byte (u8) or 16-byte (u16) load
// and store where every operand allows (VEC) and the 8 samples end inside W, sample by sample otherwise. A thread reads rec and
// the luma only at positions it alone writes when dst is rec or the luma (sx = sy = 0): in place is safe.
// Nothing outside [0, H) x [0, W) of rec and dst and outside [0, Hl) x [0, Wl) of the luma is touched.
//
// grain_stats. d = src - den; a sample counts when the four 4-neighbours of den in its own plane (indexes clamped) each differ
// from den[y][x] by at most flat << sh; its bin is bn = i >> 5. Per plane 16 uint64 words: n[0..7] the counts, S[0..7] the sums
// of d^2. A thread walks down kRows rows of one 8-sample column, den's row above, the row and the row below in registers; its
// 16 partial sums stay in registers (32-bit for u8: 32 samples x 255^2; 64-bit for u16), go through the wave (shuffles), then
// to 16 LDS words, and the workgroup issues one 64-bit integer atomic per non-zero word. Integer adds commute: the words are
// the same for every launch geometry and arrival order. One call adds less than 2^60 to a word (static_assert below).
// accumulate == 0: a first one-workgroup launch zeroes the words.
#include "ops.h"

#include <string>
#include <type_traits>

namespace dcvc {

namespace {

constexpr int kThreads = 256;
constexpr int kOut = 8;                      // consecutive samples of a thread
constexpr int kBlock = 32;                   // the blocks of the template offsets
constexpr int kTpl = 64;                     // the template's side
constexpr int kTW = 128, kTH = 64;           // grain_apply's tile
constexpr int kPasses = kTW * kTH / kOut / kThreads;
static_assert(kTW % kBlock == 0 && kTH % kBlock == 0 && kBlock % kOut == 0, "a tile holds whole blocks, a thread's samples lie in one block");
static_assert(kPasses * kOut * kThreads == kTW * kTH, "whole passes");
static_assert(kTpl * kTpl * 2 == 8192 && (kTpl * kTpl / 8) % kThreads == 0, "the template is staged in whole passes of 16-byte vectors");
static_assert(65535LL * 65535LL * kGrainMaxSide * kGrainMaxSide < (1LL << 60), "one grain_stats call adds less than 2^60 to a word");
static_assert(1023 * 255 + 512 < (1 << 18), "t v + rounding fits 32 bits with room at every depth");

constexpr int kVecCols = 32;                 // grain_stats: 8-sample columns of a tile along x
constexpr int kRows = 4;                     // ... rows a thread walks down
constexpr int kStatRows = kThreads / kVecCols * kRows;

struct Templates { const int16_t* t[3]; };
struct Luts { unsigned w[3][3]; };           // nine bytes a plane, little-endian in three words

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int absdiff(int a, int b) { return a > b ? a - b : b - a; }

// n samples (1..8) of a row from p on -> r[0..n), the rest 0; one 8- or 16-byte load where VEC says it is aligned
template <typename T, bool VEC>
__device__ __forceinline__ void load8(const T* p, int n, int (&r)[kOut])
{
    if (VEC && n == kOut) {
        if constexpr (sizeof(T) == 1) {
            const uint2 v = *reinterpret_cast<const uint2*>(p);
            const unsigned w[2] = {v.x, v.y};
#pragma unroll
            for (int e = 0; e < kOut; ++e) r[e] = static_cast<int>((w[e >> 2] >> (8 * (e & 3))) & 255u);
        } else {
            const uint4 v = *reinterpret_cast<const uint4*>(p);
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < kOut; ++e) r[e] = static_cast<int>((w[e >> 1] >> (16 * (e & 1))) & 65535u);
        }
    } else {
#pragma unroll
        for (int e = 0; e < kOut; ++e) r[e] = e < n ? static_cast<int>(p[e]) : 0;
    }
}

// the collocated luma of samples x .. x + n - 1 of a row whose luma row is lrow [Wl] -> L[0..n), the rest 0
template <typename T, int SX, bool VEC>
__device__ __forceinline__ void luma8(const T* lrow, int Wl, int x, int n, int (&L)[kOut])
{
    if constexpr (SX == 0) {
        load8<T, VEC>(lrow + x, n, L);       // x + n <= W <= Wl
    } else {
        const int lx = 2 * x;
        if (VEC && n == kOut && lx + 2 * kOut <= Wl) {
            int a[kOut], b[kOut];
            load8<T, true>(lrow + lx, kOut, a);
            load8<T, true>(lrow + lx + kOut, kOut, b);
#pragma unroll
            for (int e = 0; e < kOut / 2; ++e) {
                L[e] = (a[2 * e] + a[2 * e + 1] + 1) >> 1;
                L[e + kOut / 2] = (b[2 * e] + b[2 * e + 1] + 1) >> 1;
            }
        } else {
#pragma unroll
            for (int e = 0; e < kOut; ++e) {
                // 2 (x + e) < Wl for every sample of the plane (validated); its right neighbour may lie past the luma plane
                L[e] = e < n ? (static_cast<int>(lrow[lx + 2 * e]) + static_cast<int>(lrow[min(lx + 2 * e + 1, Wl - 1)]) + 1) >> 1 : 0;
            }
        }
    }
}

template <typename T, bool VEC>
__device__ __forceinline__ void store8(T* p, int n, const int (&o)[kOut])
{
    if (VEC && n == kOut) {
        if constexpr (sizeof(T) == 1) {
            *reinterpret_cast<uint2*>(p) = make_uint2(static_cast<unsigned>(o[0]) | (static_cast<unsigned>(o[1]) << 8) | (static_cast<unsigned>(o[2]) << 16) | (static_cast<unsigned>(o[3]) << 24),
                                                      static_cast<unsigned>(o[4]) | (static_cast<unsigned>(o[5]) << 8) | (static_cast<unsigned>(o[6]) << 16) | (static_cast<unsigned>(o[7]) << 24));
        } else {
            *reinterpret_cast<uint4*>(p) = make_uint4(static_cast<unsigned>(o[0]) | (static_cast<unsigned>(o[1]) << 16), static_cast<unsigned>(o[2]) | (static_cast<unsigned>(o[3]) << 16),
                                                      static_cast<unsigned>(o[4]) | (static_cast<unsigned>(o[5]) << 16), static_cast<unsigned>(o[6]) | (static_cast<unsigned>(o[7]) << 16));
        }
    } else {
#pragma unroll
        for (int e = 0; e < kOut; ++e) {
            if (e < n) p[e] = static_cast<T>(o[e]);
        }
    }
}

// rec, luma and dst may be one plane (see the head of the file): no __restrict__ on them
template <typename T, int SX, bool VEC>
__global__ void __launch_bounds__(kThreads)
grain_apply_kernel(const T* rec, long long rec_row_stride, long long rec_plane_stride, const T* luma, long long luma_row_stride, int Hl, int Wl,
                   T* dst, long long dst_row_stride, long long dst_plane_stride, int H, int W, int sy, int sh, int max_val, int first_plane,
                   Templates tp, Luts luts, unsigned h0, int luma_is_rec)
{
    __shared__ __attribute__((aligned(16))) int16_t tl[kTpl * kTpl];
    __shared__ int lut[9];
    const int tid = threadIdx.x;
    const int p = first_plane + static_cast<int>(blockIdx.z);
    {
        const int16_t* t = p == 0 ? tp.t[0] : (p == 1 ? tp.t[1] : tp.t[2]);
        if ((reinterpret_cast<uintptr_t>(t) & 15) == 0) {
#pragma unroll
            for (int i = 0; i < kTpl * kTpl / 8 / kThreads; ++i) {
                reinterpret_cast<uint4*>(tl)[tid + i * kThreads] = reinterpret_cast<const uint4*>(t)[tid + i * kThreads];
            }
        } else {
            for (int i = tid; i < kTpl * kTpl; i += kThreads) tl[i] = t[i];
        }
        if (tid < 9) {
            const int j = tid >> 2;
            const unsigned w0 = p == 0 ? luts.w[0][0] : (p == 1 ? luts.w[1][0] : luts.w[2][0]);
            const unsigned w1 = p == 0 ? luts.w[0][1] : (p == 1 ? luts.w[1][1] : luts.w[2][1]);
            const unsigned w2 = p == 0 ? luts.w[0][2] : (p == 1 ? luts.w[1][2] : luts.w[2][2]);
            const unsigned w = j == 0 ? w0 : (j == 1 ? w1 : w2);
            lut[tid] = static_cast<int>((w >> (8 * (tid & 3))) & 255u);
        }
    }
    __syncthreads();
    const T* rp = rec + static_cast<long long>(blockIdx.z) * rec_plane_stride;
    T* dp = dst + static_cast<long long>(blockIdx.z) * dst_plane_stride;
    const unsigned hp = h0 + static_cast<unsigned>(p) * 0xC2B2AE3Du;
    const int round = 1 << (9 - sh), shift = 10 - sh;
#pragma unroll 1
    for (int pass = 0; pass < kPasses; ++pass) {
        const int slot = tid + pass * kThreads;
        const int y = blockIdx.y * kTH + slot / (kTW / kOut), x = blockIdx.x * kTW + (slot % (kTW / kOut)) * kOut;
        if (y >= H || x >= W) continue;
        const int n = min(kOut, W - x);
        unsigned h = hp + static_cast<unsigned>(y >> 5) * 0x27D4EB2Fu + static_cast<unsigned>(x >> 5) * 0x165667B1u;
        h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
        const int ox = static_cast<int>(h & 63u), oy = static_cast<int>((h >> 8) & 63u);
        const int16_t* trow = tl + ((oy + (y & 31)) & 63) * kTpl;
        const int tc = ox + (x & 31);
        int R[kOut], L[kOut], o[kOut];
        load8<T, VEC>(rp + static_cast<long long>(y) * rec_row_stride + x, n, R);
        if (luma_is_rec) {
#pragma unroll
            for (int e = 0; e < kOut; ++e) L[e] = R[e];
        } else {
            luma8<T, SX, VEC>(luma + static_cast<long long>(min(y << sy, Hl - 1)) * luma_row_stride, Wl, x, n, L);
        }
#pragma unroll
        for (int e = 0; e < kOut; ++e) {
            const int t = trow[(tc + e) & 63];
            const int i = min(L[e] >> sh, 255), k = i >> 5, fr = i & 31;
            const int v = (lut[k] * (32 - fr) + lut[k + 1] * fr + 16) >> 5;
            o[e] = clampi(R[e] + ((t * v + round) >> shift), 0, max_val);
        }
        store8<T, VEC>(dp + static_cast<long long>(y) * dst_row_stride + x, n, o);
    }
}

template <typename A> __device__ __forceinline__ A wave_sum(A v);
template <> __device__ __forceinline__ unsigned wave_sum<unsigned>(unsigned v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}
template <> __device__ __forceinline__ unsigned long long wave_sum<unsigned long long>(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_down(static_cast<unsigned>(v), o), hi = __shfl_down(static_cast<unsigned>(v >> 32), o);
        v += (static_cast<unsigned long long>(hi) << 32) | lo;
    }
    return v;
}

__global__ void grain_stats_zero_kernel(unsigned long long* __restrict__ words) { words[threadIdx.x] = 0ull; }

template <typename T, int SX, bool VEC>
__global__ void __launch_bounds__(kThreads)
grain_stats_kernel(const T* __restrict__ src, long long src_row_stride, long long src_plane_stride, const T* __restrict__ den,
                   long long den_row_stride, long long den_plane_stride, const T* __restrict__ luma, long long luma_row_stride, int Hl,
                   int Wl, int H, int W, int sy, int sh, int flat, int luma_is_den, unsigned long long* __restrict__ words)
{
    using Acc = typename std::conditional<sizeof(T) == 1, unsigned, unsigned long long>::type;      // 32 samples of 255^2 fit 32 bits
    static_assert(sizeof(T) == 2 || 255LL * 255 * kRows * kOut * 64 < (1LL << 32), "u8: a wave's partial sums fit 32 bits");
    __shared__ unsigned long long part[16];
    const int tid = threadIdx.x, tx = tid % kVecCols, ty = tid / kVecCols;
    if (tid < 16) part[tid] = 0ull;
    __syncthreads();
    const int x = blockIdx.x * (kVecCols * kOut) + tx * kOut, y0 = blockIdx.y * kStatRows + ty * kRows;
    const int n = min(kOut, W - x);          // <= 0: the column lies past the plane
    unsigned cnt[8] = {};
    Acc sum[8] = {};
    if (n > 0 && y0 < H) {
        const T* sp = src + static_cast<long long>(blockIdx.z) * src_plane_stride + x;
        const T* dn = den + static_cast<long long>(blockIdx.z) * den_plane_stride;
        const T* dp = dn + x;
        const int xl = max(x - 1, 0), xr = min(x + kOut, W - 1);      // the columns left and right of the thread's samples, clamped
        const int lim = flat << sh;
        int a[kOut], c[kOut], b[kOut], s[kOut], L[kOut];
        load8<T, VEC>(dp + static_cast<long long>(max(y0 - 1, 0)) * den_row_stride, n, a);
        load8<T, VEC>(dp + static_cast<long long>(y0) * den_row_stride, n, c);
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int y = y0 + r;
            if (y >= H) break;
            load8<T, VEC>(dp + static_cast<long long>(min(y + 1, H - 1)) * den_row_stride, n, b);
            load8<T, VEC>(sp + static_cast<long long>(y) * src_row_stride, n, s);
            const T* drow = dn + static_cast<long long>(y) * den_row_stride;
            const int left = drow[xl], right = drow[xr];
            if (luma_is_den) {
#pragma unroll
                for (int e = 0; e < kOut; ++e) L[e] = c[e];
            } else {
                luma8<T, SX, VEC>(luma + static_cast<long long>(min(y << sy, Hl - 1)) * luma_row_stride, Wl, x, n, L);
            }
#pragma unroll
            for (int e = 0; e < kOut; ++e) {
                const int l = e == 0 ? left : c[e - 1];
                // the right neighbour: the next sample; past the thread's eight, the column to their right; past the plane, the sample itself
                const int rr = e + 1 < n ? c[e + 1 < kOut ? e + 1 : e] : (n == kOut ? right : c[e]);
                const bool ok = e < n && absdiff(a[e], c[e]) <= lim && absdiff(b[e], c[e]) <= lim && absdiff(l, c[e]) <= lim && absdiff(rr, c[e]) <= lim;
                const unsigned d = static_cast<unsigned>(absdiff(s[e], c[e]));
                const unsigned dd = d * d;                             // |d| <= 65535: d^2 < 2^32 as unsigned
                const int bn = min(L[e] >> sh, 255) >> 5;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const bool hit = ok && bn == k;
                    cnt[k] += hit ? 1u : 0u;
                    sum[k] += hit ? static_cast<Acc>(dd) : static_cast<Acc>(0);
                }
            }
#pragma unroll
            for (int e = 0; e < kOut; ++e) { a[e] = c[e]; c[e] = b[e]; }
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const unsigned nk = wave_sum<unsigned>(cnt[k]);
        const Acc sk = wave_sum<Acc>(sum[k]);
        if ((tid & 63) == 0) {
            if (nk) atomicAdd(&part[k], static_cast<unsigned long long>(nk));
            if (sk) atomicAdd(&part[8 + k], static_cast<unsigned long long>(sk));
        }
    }
    __syncthreads();
    if (tid < 16) {
        const unsigned long long v = part[tid];
        if (v) atomicAdd(words + 16 * blockIdx.z + tid, v);
    }
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// [lo, hi) in bytes of n planes of h rows of w samples
void extent(const void* p, int es, int n, int h, int w, long long row_stride, long long plane_stride, uintptr_t& lo, uintptr_t& hi)
{
    lo = reinterpret_cast<uintptr_t>(p);
    hi = lo + static_cast<uintptr_t>((n - 1) * plane_stride + (h - 1) * row_stride + w) * static_cast<uintptr_t>(es);
}

bool overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

// what both entries refuse alike; `who` names the kernel in the message. Returns the bytes of a sample
int common_checks(const std::string& k, int dtype, int bit_depth, int H, int W, int sx, int sy, int Hl, int Wl, int luma_row_stride)
{
    if (dtype != kSampleU8 && dtype != kSampleU16) throw std::invalid_argument(k + ": the sample type must be DCVC_SAMPLE_U8 or DCVC_SAMPLE_U16");
    const int es = dtype == kSampleU8 ? 1 : 2;
    if (es == 1 ? bit_depth != 8 : (bit_depth < 9 || bit_depth > 16)) {
        throw std::invalid_argument(k + ": bit_depth must be 8 (u8) or 9..16 (u16), got " + std::to_string(bit_depth));
    }
    if (H < 1 || W < 1 || H > kGrainMaxSide || W > kGrainMaxSide) {
        throw std::invalid_argument(k + ": sides must be in 1.." + std::to_string(kGrainMaxSide) + ", got " + std::to_string(W) + "x" + std::to_string(H));
    }
    if (sx < 0 || sx > 1 || sy < 0 || sy > 1) {
        throw std::invalid_argument(k + ": sx and sy must be 0 or 1, got " + std::to_string(sx) + ", " + std::to_string(sy));
    }
    const int need_h = ((H - 1) << sy) + 1, need_w = ((W - 1) << sx) + 1;
    if (Hl < need_h || Wl < need_w || Hl > 2 * kGrainMaxSide || Wl > 2 * kGrainMaxSide) {
        throw std::invalid_argument(k + ": the luma plane must be " + std::to_string(need_w) + "x" + std::to_string(need_h) + " up to " +
                                    std::to_string(2 * kGrainMaxSide) + " a side, got " + std::to_string(Wl) + "x" + std::to_string(Hl));
    }
    if (luma_row_stride < Wl) throw std::invalid_argument(k + ": a row stride is below the width");
    return es;
}

template <typename T, int SX>
void launch_apply(const GrainApplyDesc& d, hipStream_t stream)
{
    const bool one = d.n_planes == 1;
    constexpr size_t a = kOut * sizeof(T);
    auto fits = [&](const void* p, long long row_stride, long long plane_stride, size_t al) {
        return aligned(p, al) && (row_stride * sizeof(T)) % al == 0 && (one || (plane_stride * sizeof(T)) % al == 0);
    };
    const bool same = d.luma == d.rec && d.sx == 0 && d.sy == 0 && one && d.luma_row_stride == d.rec_row_stride;
    const bool vec = fits(d.rec, d.rec_row_stride, d.rec_plane_stride, a) && fits(d.dst, d.dst_row_stride, d.dst_plane_stride, a) &&
                     (same || (aligned(d.luma, a) && (d.luma_row_stride * sizeof(T)) % a == 0));
    Templates tp;
    Luts luts;
    for (int p = 0; p < 3; ++p) {
        tp.t[p] = d.templates[p];
        for (int j = 0; j < 3; ++j) luts.w[p][j] = 0u;
        for (int j = 0; j < 9; ++j) luts.w[p][j >> 2] |= static_cast<unsigned>(d.lut[p * 9 + j]) << (8 * (j & 3));
    }
    const unsigned h0 = d.seed * 0x9E3779B1u + d.pic * 0x85EBCA77u;
    const int sh = d.bit_depth - 8;
    const dim3 grid((d.W + kTW - 1) / kTW, (d.H + kTH - 1) / kTH, d.n_planes);
    auto k = vec ? grain_apply_kernel<T, SX, true> : grain_apply_kernel<T, SX, false>;
    hipLaunchKernelGGL(k, grid, dim3(kThreads), 0, stream, static_cast<const T*>(d.rec), static_cast<long long>(d.rec_row_stride),
                       d.rec_plane_stride, static_cast<const T*>(d.luma), static_cast<long long>(d.luma_row_stride), d.Hl, d.Wl,
                       static_cast<T*>(d.dst), static_cast<long long>(d.dst_row_stride), d.dst_plane_stride, d.H, d.W, d.sy, sh,
                       (1 << d.bit_depth) - 1, d.first_plane, tp, luts, h0, same ? 1 : 0);
    hip_check(hipGetLastError(), "grain_apply launch");
}

template <typename T, int SX>
void launch_stats(const GrainStatsDesc& d, hipStream_t stream)
{
    const bool one = d.n_planes == 1;
    constexpr size_t a = kOut * sizeof(T);
    auto fits = [&](const void* p, long long row_stride, long long plane_stride) {
        return aligned(p, a) && (row_stride * sizeof(T)) % a == 0 && (one || (plane_stride * sizeof(T)) % a == 0);
    };
    const bool same = d.luma == d.den && d.sx == 0 && d.sy == 0 && one && d.luma_row_stride == d.den_row_stride;
    const bool vec = fits(d.src, d.src_row_stride, d.src_plane_stride) && fits(d.den, d.den_row_stride, d.den_plane_stride) &&
                     (same || (aligned(d.luma, a) && (d.luma_row_stride * sizeof(T)) % a == 0));
    unsigned long long* words = static_cast<unsigned long long*>(d.words);
    if (!d.accumulate) {
        hipLaunchKernelGGL(grain_stats_zero_kernel, dim3(1), dim3(16 * d.n_planes), 0, stream, words);
        hip_check(hipGetLastError(), "grain_stats zero launch");
    }
    const dim3 grid((d.W + kVecCols * kOut - 1) / (kVecCols * kOut), (d.H + kStatRows - 1) / kStatRows, d.n_planes);
    auto k = vec ? grain_stats_kernel<T, SX, true> : grain_stats_kernel<T, SX, false>;
    hipLaunchKernelGGL(k, grid, dim3(kThreads), 0, stream, static_cast<const T*>(d.src), static_cast<long long>(d.src_row_stride),
                       d.src_plane_stride, static_cast<const T*>(d.den), static_cast<long long>(d.den_row_stride), d.den_plane_stride,
                       static_cast<const T*>(d.luma), static_cast<long long>(d.luma_row_stride), d.Hl, d.Wl, d.H, d.W, d.sy,
                       d.bit_depth - 8, d.flat, same ? 1 : 0, words);
    hip_check(hipGetLastError(), "grain_stats launch");
}

}  // namespace

void grain_apply_validate(const GrainApplyDesc& d)
{
    const std::string k = "grain_apply";
    if (d.rec == nullptr || d.luma == nullptr || d.dst == nullptr || d.lut == nullptr) throw std::invalid_argument(k + ": null operand");
    const int es = common_checks(k, d.dtype, d.bit_depth, d.H, d.W, d.sx, d.sy, d.Hl, d.Wl, d.luma_row_stride);
    if (d.n_planes < 1 || d.n_planes > 3 || d.first_plane < 0 || d.first_plane + d.n_planes > 3) {
        throw std::invalid_argument(k + ": n_planes must be in 1..3 and first_plane + n_planes at most 3, got " + std::to_string(d.n_planes) +
                                    " from " + std::to_string(d.first_plane));
    }
    for (int p = d.first_plane; p < d.first_plane + d.n_planes; ++p) {
        if (d.templates[p] == nullptr) throw std::invalid_argument(k + ": null template of plane " + std::to_string(p));
        if (!aligned(d.templates[p], 2)) throw std::invalid_argument(k + ": templates must be 2-byte aligned");
    }
    const long long plane = static_cast<long long>(d.H - 1);
    if (d.rec_row_stride < d.W || d.dst_row_stride < d.W) throw std::invalid_argument(k + ": a row stride is below the width");
    if (d.n_planes > 1 && (d.rec_plane_stride < plane * d.rec_row_stride + d.W || d.dst_plane_stride < plane * d.dst_row_stride + d.W)) {
        throw std::invalid_argument(k + ": a plane stride is below the plane");
    }
    if (!aligned(d.rec, es) || !aligned(d.luma, es) || !aligned(d.dst, es)) throw std::invalid_argument(k + ": 16-bit planes must be 2-byte aligned");
    uintptr_t r0, r1, l0, l1, d0, d1;
    extent(d.rec, es, d.n_planes, d.H, d.W, d.rec_row_stride, d.rec_plane_stride, r0, r1);
    extent(d.luma, es, 1, d.Hl, d.Wl, d.luma_row_stride, 0, l0, l1);
    extent(d.dst, es, d.n_planes, d.H, d.W, d.dst_row_stride, d.dst_plane_stride, d0, d1);
    const bool in_place = d.dst == d.rec && d.dst_row_stride == d.rec_row_stride && (d.n_planes == 1 || d.dst_plane_stride == d.rec_plane_stride);
    if (!in_place && overlap(r0, r1, d0, d1)) throw std::invalid_argument(k + ": dst overlaps rec (dst may be rec itself, strided likewise)");
    // the luma must stay the ungrained reconstruction while any plane reads it: dst may hold it only when it is the one plane
    // of the call, every sample's luma its own position
    const bool luma_is_rec = d.luma == d.rec && d.luma_row_stride == d.rec_row_stride && d.sx == 0 && d.sy == 0 && d.n_planes == 1;
    if (overlap(l0, l1, d0, d1) && !(luma_is_rec && in_place)) {
        throw std::invalid_argument(k + ": dst overlaps the luma plane (allowed for one plane that is rec and the luma with sx = sy = 0)");
    }
    for (int p = d.first_plane; p < d.first_plane + d.n_planes; ++p) {
        const uintptr_t t0 = reinterpret_cast<uintptr_t>(d.templates[p]);
        if (overlap(t0, t0 + kTpl * kTpl * 2, d0, d1)) throw std::invalid_argument(k + ": dst overlaps a template");
    }
}

void grain_apply(const GrainApplyDesc& d, hipStream_t stream)
{
    grain_apply_validate(d);
    if (d.dtype == kSampleU8) {
        if (d.sx) launch_apply<uint8_t, 1>(d, stream); else launch_apply<uint8_t, 0>(d, stream);
    } else {
        if (d.sx) launch_apply<uint16_t, 1>(d, stream); else launch_apply<uint16_t, 0>(d, stream);
    }
}

void grain_stats_validate(const GrainStatsDesc& d)
{
    const std::string k = "grain_stats";
    if (d.src == nullptr || d.den == nullptr || d.luma == nullptr || d.words == nullptr) throw std::invalid_argument(k + ": null operand");
    const int es = common_checks(k, d.dtype, d.bit_depth, d.H, d.W, d.sx, d.sy, d.Hl, d.Wl, d.luma_row_stride);
    if (d.n_planes < 1 || d.n_planes > 2) throw std::invalid_argument(k + ": n_planes must be 1 or 2, got " + std::to_string(d.n_planes));
    if (d.flat < 0 || d.flat > 255) throw std::invalid_argument(k + ": flat must be in 0..255, got " + std::to_string(d.flat));
    if (d.accumulate < 0 || d.accumulate > 1) throw std::invalid_argument(k + ": accumulate must be 0 or 1, got " + std::to_string(d.accumulate));
    const long long plane = static_cast<long long>(d.H - 1);
    if (d.src_row_stride < d.W || d.den_row_stride < d.W) throw std::invalid_argument(k + ": a row stride is below the width");
    if (d.n_planes > 1 && (d.src_plane_stride < plane * d.src_row_stride + d.W || d.den_plane_stride < plane * d.den_row_stride + d.W)) {
        throw std::invalid_argument(k + ": a plane stride is below the plane");
    }
    if (!aligned(d.src, es) || !aligned(d.den, es) || !aligned(d.luma, es)) throw std::invalid_argument(k + ": 16-bit planes must be 2-byte aligned");
    if (!aligned(d.words, 8)) throw std::invalid_argument(k + ": words must be 8-byte aligned");
}

void grain_stats(const GrainStatsDesc& d, hipStream_t stream)
{
    grain_stats_validate(d);
    if (d.dtype == kSampleU8) {
        if (d.sx) launch_stats<uint8_t, 1>(d, stream); else launch_stats<uint8_t, 0>(d, stream);
    } else {
        if (d.sx) launch_stats<uint16_t, 1>(d, stream); else launch_stats<uint16_t, 0>(d, stream);
    }
}

}  // namespace dcvc
