// msssim.hip - MS-SSIM of a batch of equal-sized planes on the GPU (src/utils/metrics.py:27-91 calc_msssim).
//
// The reference runs the metric on the host in float64: an 11 x 11 Gaussian (sigma 1.5, fspecial_gauss) through
// scipy.signal.fftconvolve over the valid region, K1 = 0.01, K2 = 0.03, data range 255, the mean of the ssim and cs maps
// per level, a 2 x 2 block mean (ndimage.convolve mode='reflect', then [::2, ::2]: the last row / column replicated when a
// side is odd) between levels, and prod(cs[0:L-1] ** w[0:L-1]) * ssim[L-1] ** w[L-1] over 5 levels (4 when a side is
// below 176). A data range other than 255 (high-bit-depth samples) only changes C1 and C2, computed in fp64 from it.
// Here everything after the load is fp64 too: the Gaussian is applied as two 11-tap passes (it is separable),
// which agrees with the reference's FFT to a few 1e-15; fp32 would be off by ~1e-6, visible in the log.
//
// One launch per pyramid level for all planes (blockIdx.z = plane): a workgroup loads a 16 x 32 output tile plus its
// 10-sample halo of both planes into LDS as fp64, runs the horizontal pass into five moment tiles (x, y, x^2, y^2, xy), the
// vertical pass from there, and writes one (ssim, cs) partial-sum pair per workgroup; the same launch writes the 2 x 2
// averaged planes of the next level (grid-stride, independent of the tiles). A last launch (one workgroup per plane)
// reduces the partial sums in a fixed order and evaluates the formula. No atomics: results are bitwise reproducible.
#include "ops.h"

#include <cmath>

namespace dcvc {

namespace {

constexpr int kTH = 16, kTW = 32;               // output tile
constexpr int kTaps = 11, kHalo = kTaps - 1;
constexpr int kInH = kTH + kHalo, kInW = kTW + kHalo;
constexpr int kThreads = 256;
constexpr int kMaxLevels = 5;

struct Taps {
    double g[kTaps];
    double c1, c2;      // (K1 data_range)^2, (K2 data_range)^2
};

__device__ __forceinline__ double sample(const uint8_t* p, long long i) { return static_cast<double>(p[i]); }
__device__ __forceinline__ double sample(const half_t* p, long long i) { return static_cast<double>(static_cast<float>(p[i])); }
__device__ __forceinline__ double sample(const uint16_t* p, long long i) { return static_cast<double>(p[i]); }
__device__ __forceinline__ double sample(const float* p, long long i) { return static_cast<double>(p[i]); }
__device__ __forceinline__ double sample(const double* p, long long i) { return p[i]; }

// fixed-order sum of one value per thread over the workgroup (256 threads = 4 waves); the result is valid in thread 0
__device__ __forceinline__ double2 block_sum(double2 v, double2* scratch)
{
    for (int o = 32; o > 0; o >>= 1) {
        v.x += __shfl_down(v.x, o);
        v.y += __shfl_down(v.y, o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    double2 s = make_double2(0.0, 0.0);
    if (threadIdx.x == 0) {
        for (int i = 0; i < kThreads / 64; ++i) {
            s.x += scratch[i].x;
            s.y += scratch[i].y;
        }
    }
    __syncthreads();
    return s;
}

// One pyramid level. a / b: plane p starts at p * plane_stride, row r at r * row_stride (samples). partial: [planes][tiles]
// (ssim sum, cs sum) over the tile's valid outputs. next_a / next_b: [planes][ceil(h/2)][ceil(w/2)], or null at the last level.
template <typename TA, typename TB>
__global__ void __launch_bounds__(kThreads) msssim_level_kernel(const TA* __restrict__ a, const TB* __restrict__ b, int h, int w,
                                                                long long row_stride, long long plane_stride, Taps taps,
                                                                double2* __restrict__ partial, double* __restrict__ next_a,
                                                                double* __restrict__ next_b)
{
    __shared__ double xa[kInH][kInW], xb[kInH][kInW];
    __shared__ double mom[5][kInH][kTW];
    __shared__ double2 red[kThreads / 64];

    const int tid = threadIdx.x, p = blockIdx.z;
    const int tiles = gridDim.x * gridDim.y, tile = blockIdx.y * gridDim.x + blockIdx.x;
    const TA* pa = a + p * plane_stride;
    const TB* pb = b + p * plane_stride;

    // the next level's planes: 2 x 2 block mean, last row / column replicated on an odd side
    if (next_a != nullptr) {
        const int nh = (h + 1) >> 1, nw = (w + 1) >> 1;
        const long long n = static_cast<long long>(nh) * nw;
        double* oa = next_a + p * n;
        double* ob = next_b + p * n;
        for (long long i = static_cast<long long>(tile) * kThreads + tid; i < n; i += static_cast<long long>(tiles) * kThreads) {
            const int r = static_cast<int>(i / nw), c = static_cast<int>(i - static_cast<long long>(r) * nw);
            const long long o00 = 2LL * r * row_stride + 2 * c;
            const long long dr = 2 * r + 1 < h ? row_stride : 0, dc = 2 * c + 1 < w ? 1 : 0;
            oa[i] = (((sample(pa, o00) + sample(pa, o00 + dc)) + sample(pa, o00 + dr)) + sample(pa, o00 + dr + dc)) * 0.25;
            ob[i] = (((sample(pb, o00) + sample(pb, o00 + dc)) + sample(pb, o00 + dr)) + sample(pb, o00 + dr + dc)) * 0.25;
        }
    }

    // tile + halo of both planes; reads beyond the plane are clamped to its last row / column (they only feed outputs
    // outside the valid region, which are not summed)
    const int r0 = blockIdx.y * kTH, c0 = blockIdx.x * kTW;
    for (int i = tid; i < kInH * kInW; i += kThreads) {
        const int r = i / kInW, c = i - r * kInW;
        const long long o = static_cast<long long>(min(r0 + r, h - 1)) * row_stride + min(c0 + c, w - 1);
        xa[r][c] = sample(pa, o);
        xb[r][c] = sample(pb, o);
    }
    __syncthreads();

    // horizontal pass: the five moments of every input row of the tile at the tile's output columns
    for (int i = tid; i < kInH * kTW; i += kThreads) {
        const int r = i / kTW, c = i - r * kTW;
        double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            const double x = xa[r][c + k], y = xb[r][c + k];
            const double gx = taps.g[k] * x, gy = taps.g[k] * y;
            sx += gx;
            sy += gy;
            sxx = fma(gx, x, sxx);
            syy = fma(gy, y, syy);
            sxy = fma(gx, y, sxy);
        }
        mom[0][r][c] = sx;
        mom[1][r][c] = sy;
        mom[2][r][c] = sxx;
        mom[3][r][c] = syy;
        mom[4][r][c] = sxy;
    }
    __syncthreads();

    // vertical pass + the ssim / cs maps (written as the reference writes them: identical planes give exactly 1)
    const int oh = h - kHalo, ow = w - kHalo;
    const int c = tid % kTW;
    double2 acc = make_double2(0.0, 0.0);
    for (int r = tid / kTW; r < kTH; r += kThreads / kTW) {
        if (r0 + r >= oh || c0 + c >= ow) continue;
        double mu1 = 0, mu2 = 0, exx = 0, eyy = 0, exy = 0;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            const double g = taps.g[k];
            mu1 = fma(g, mom[0][r + k][c], mu1);
            mu2 = fma(g, mom[1][r + k][c], mu2);
            exx = fma(g, mom[2][r + k][c], exx);
            eyy = fma(g, mom[3][r + k][c], eyy);
            exy = fma(g, mom[4][r + k][c], exy);
        }
        const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
        const double s1 = exx - mu1_sq, s2 = eyy - mu2_sq, s12 = exy - mu1_mu2;
        const double num_cs = 2 * s12 + taps.c2, den_cs = s1 + s2 + taps.c2;
        acc.x += ((2 * mu1_mu2 + taps.c1) * num_cs) / ((mu1_sq + mu2_sq + taps.c1) * den_cs);
        acc.y += num_cs / den_cs;
    }
    const double2 s = block_sum(acc, red);
    if (tid == 0) partial[static_cast<long long>(p) * tiles + tile] = s;
}

struct LevelSums {
    int levels = 0;
    long long offset[kMaxLevels];      // first partial of the level (plane 0)
    int tiles[kMaxLevels];             // partials per plane
    double count[kMaxLevels];          // valid outputs per plane
    double weight[kMaxLevels];
};

// one workgroup per plane: mean ssim / cs of every level (fixed-order sums), then the MS-SSIM formula
__global__ void __launch_bounds__(kThreads) msssim_final_kernel(const double2* __restrict__ partial, LevelSums ls,
                                                                double* __restrict__ out)
{
    __shared__ double2 red[kThreads / 64];
    const int p = blockIdx.x;
    double ms = 0, mc = 0;          // thread 0: the last level's ssim mean; running product of the cs terms
    double prod = 1.0;
    for (int l = 0; l < ls.levels; ++l) {
        const double2* q = partial + ls.offset[l] + static_cast<long long>(p) * ls.tiles[l];
        double2 v = make_double2(0.0, 0.0);
        for (int i = threadIdx.x; i < ls.tiles[l]; i += kThreads) {
            v.x += q[i].x;
            v.y += q[i].y;
        }
        const double2 s = block_sum(v, red);
        if (threadIdx.x == 0) {
            ms = s.x / ls.count[l];
            mc = s.y / ls.count[l];
            // numpy: mcs ** w is NaN for a negative cs mean - kept, not clamped
            if (l < ls.levels - 1) prod = l == 0 ? pow(mc, ls.weight[l]) : prod * pow(mc, ls.weight[l]);
        }
    }
    if (threadIdx.x == 0) out[p] = prod * pow(ms, ls.weight[ls.levels - 1]);
}

struct Pyramid {
    int levels = 0;
    int h[kMaxLevels], w[kMaxLevels];
    size_t plane_off[kMaxLevels];      // doubles: level l >= 1, src planes at plane_off[l], rec planes behind them
    long long partial_off[kMaxLevels]; // double2 units, behind the planes
    int tiles_x[kMaxLevels], tiles_y[kMaxLevels];
    size_t bytes = 0;
};

Pyramid pyramid(int n_planes, int H, int W)
{
    Pyramid py;
    py.levels = (H < 176 || W < 176) ? 4 : 5;
    size_t doubles = 0;
    for (int l = 0; l < py.levels; ++l) {
        py.h[l] = l == 0 ? H : (py.h[l - 1] + 1) / 2;
        py.w[l] = l == 0 ? W : (py.w[l - 1] + 1) / 2;
        py.tiles_x[l] = (py.w[l] - kHalo + kTW - 1) / kTW;
        py.tiles_y[l] = (py.h[l] - kHalo + kTH - 1) / kTH;
        py.plane_off[l] = doubles;
        if (l > 0) doubles += 2ull * n_planes * py.h[l] * py.w[l];
    }
    long long pairs = 0;
    for (int l = 0; l < py.levels; ++l) {
        py.partial_off[l] = pairs;
        pairs += static_cast<long long>(n_planes) * py.tiles_x[l] * py.tiles_y[l];
    }
    doubles = (doubles + 1) & ~static_cast<size_t>(1);      // 16-B alignment of the partials
    py.bytes = doubles * 8 + static_cast<size_t>(pairs) * 16;
    for (int l = 0; l < py.levels; ++l) py.partial_off[l] += static_cast<long long>(doubles / 2);
    return py;
}

Taps gauss_taps(double data_range)
{
    // fspecial_gauss(11, 1.5) = e(x) e(y) / sum: the outer product of e / sum(e) with itself
    Taps t;
    double s = 0;
    for (int k = 0; k < kTaps; ++k) {
        const double d = k - kTaps / 2;
        t.g[k] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
        s += t.g[k];
    }
    for (int k = 0; k < kTaps; ++k) t.g[k] /= s;
    t.c1 = (0.01 * data_range) * (0.01 * data_range);
    t.c2 = (0.03 * data_range) * (0.03 * data_range);
    return t;
}

template <typename TA, typename TB>
void launch_level(const TA* a, const TB* b, int n_planes, int h, int w, long long row_stride, long long plane_stride,
                  int tx, int ty, double2* partial, double* next_a, double* next_b, const Taps& taps, hipStream_t stream)
{
    hipLaunchKernelGGL((msssim_level_kernel<TA, TB>), dim3(tx, ty, n_planes), dim3(kThreads), 0, stream, a, b, h, w, row_stride,
                       plane_stride, taps, partial, next_a, next_b);
    hip_check(hipGetLastError(), "msssim level launch");
}

template <typename TA>
void launch_level0(const TA* a, const void* b, int b_dtype, int n_planes, int h, int w, long long row_stride,
                   long long plane_stride, int tx, int ty, double2* partial, double* next_a, double* next_b, const Taps& taps,
                   hipStream_t stream)
{
#define LEVEL0(TB) launch_level(a, static_cast<const TB*>(b), n_planes, h, w, row_stride, plane_stride, tx, ty, partial, next_a, \
                               next_b, taps, stream)
    switch (b_dtype) {
    case kSampleU8: LEVEL0(uint8_t); break;
    case kSampleF16: LEVEL0(half_t); break;
    case kSampleU16: LEVEL0(uint16_t); break;
    default: LEVEL0(float); break;
    }
#undef LEVEL0
}

}  // namespace

size_t msssim_workspace_bytes(int n_planes, int H, int W)
{
    return pyramid(n_planes, H, W).bytes;
}

void msssim_validate(const MsssimDesc& d)
{
    if (d.H < 88 || d.W < 88) throw std::invalid_argument("msssim: both sides must be at least 88 samples (metrics.py asserts)");
    if (d.n_planes < 1 || d.n_planes > 65535) throw std::invalid_argument("msssim: 1 to 65535 planes");
    if (!known_sample(d.src_dtype) || !known_sample(d.rec_dtype)) {
        throw std::invalid_argument("msssim: sample type must be DCVC_SAMPLE_U8, _F16, _U16 or _F32");
    }
    if (!(d.data_range > 0) || std::isinf(d.data_range)) throw std::invalid_argument("msssim: data_range must be positive and finite");
    if (d.row_stride < d.W) throw std::invalid_argument("msssim: row_stride must be >= W");
    if (d.n_planes > 1 && d.plane_stride < static_cast<long long>(d.H - 1) * d.row_stride + d.W) {
        throw std::invalid_argument("msssim: planes overlap (plane_stride < (H - 1) * row_stride + W)");
    }
    if (!d.src || !d.rec || !d.out) throw std::invalid_argument("msssim: missing operand");
}

void msssim(const MsssimDesc& d, void* workspace, hipStream_t stream)
{
    msssim_validate(d);
    if (!workspace) throw std::invalid_argument("msssim: missing workspace");
    const Pyramid py = pyramid(d.n_planes, d.H, d.W);
    double* ws = static_cast<double*>(workspace);
    double2* partial = reinterpret_cast<double2*>(ws);
    const Taps taps = gauss_taps(d.data_range);
    LevelSums ls;
    ls.levels = py.levels;
    static const double w5[5] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333}, w4[4] = {0.0517, 0.3295, 0.3462, 0.2726};
    for (int l = 0; l < py.levels; ++l) {
        const bool last = l == py.levels - 1;
        const long long n_next = last ? 0 : static_cast<long long>(py.h[l + 1]) * py.w[l + 1];
        double* na = last ? nullptr : ws + py.plane_off[l + 1];
        double* nb = last ? nullptr : na + d.n_planes * n_next;
        double2* part = partial + py.partial_off[l];
        if (l == 0) {
#define LEVEL0(TA) launch_level0(static_cast<const TA*>(d.src), d.rec, d.rec_dtype, d.n_planes, d.H, d.W, d.row_stride, \
                                 d.plane_stride, py.tiles_x[0], py.tiles_y[0], part, na, nb, taps, stream)
            switch (d.src_dtype) {
            case kSampleU8: LEVEL0(uint8_t); break;
            case kSampleF16: LEVEL0(half_t); break;
            case kSampleU16: LEVEL0(uint16_t); break;
            default: LEVEL0(float); break;
            }
#undef LEVEL0
        } else {
            const long long n = static_cast<long long>(py.h[l]) * py.w[l];
            const double* a = ws + py.plane_off[l];
            launch_level(a, a + d.n_planes * n, d.n_planes, py.h[l], py.w[l], py.w[l], n, py.tiles_x[l], py.tiles_y[l], part, na, nb,
                         taps, stream);
        }
        ls.offset[l] = py.partial_off[l];
        ls.tiles[l] = py.tiles_x[l] * py.tiles_y[l];
        ls.count[l] = static_cast<double>(py.h[l] - kHalo) * (py.w[l] - kHalo);
        ls.weight[l] = py.levels == 5 ? w5[l] : w4[l];
    }
    hipLaunchKernelGGL(msssim_final_kernel, dim3(d.n_planes), dim3(kThreads), 0, stream, partial, ls, d.out);
    hip_check(hipGetLastError(), "msssim final launch");
}

}  // namespace dcvc
