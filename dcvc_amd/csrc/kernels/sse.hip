// sse.hip - the fp64 sum of squared differences behind the PSNRs (metrics.py:10-24 calc_psnr: an fp64 mean square), on the GPU.
//
// One thread per 8 samples of a row, 8- / 16-byte loads where the rows allow them. One fp64 partial per workgroup, reduced
// by a second launch in a fixed order: no atomics, the result is bitwise reproducible and independent of how many planes
// one call covers.
#include "arith.h"
#include "picture_io.h"

namespace dcvc {

namespace {

constexpr int kThreads = kPictureThreads;
constexpr int kSsePartials = 1024;       // most workgroups per plane of the sum of squares (a function of H, W alone)

__device__ __forceinline__ double sample(uint8_t v) { return static_cast<double>(v); }
__device__ __forceinline__ double sample(half_t v) { return static_cast<double>(static_cast<float>(v)); }
__device__ __forceinline__ double sample(uint16_t v) { return static_cast<double>(v); }
__device__ __forceinline__ double sample(float v) { return static_cast<double>(v); }

// 8 samples in one access (u8: 8 B; fp16, u16: 16 B) or two (fp32: 2 x 16 B)
template <typename T> struct Vec8 { T v[8]; };
template <typename T> __device__ __forceinline__ Vec8<T> load8(const T* p)
{
    Vec8<T> r;
    if constexpr (sizeof(T) == 1) {
        *reinterpret_cast<uint2*>(r.v) = *reinterpret_cast<const uint2*>(p);
    } else if constexpr (sizeof(T) == 2) {
        *reinterpret_cast<uint4*>(r.v) = *reinterpret_cast<const uint4*>(p);
    } else {
        reinterpret_cast<uint4*>(r.v)[0] = reinterpret_cast<const uint4*>(p)[0];
        reinterpret_cast<uint4*>(r.v)[1] = reinterpret_cast<const uint4*>(p)[1];
    }
    return r;
}

// fixed-order sum over the workgroup (256 threads = 4 waves); valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* scratch)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
        for (int k = 0; k < kThreads / 64; ++k) s += scratch[k];
    }
    return s;
}

// partial[plane][blockIdx.x]: the squared differences of 8-sample row pieces blockIdx.x, + gridDim.x, ... of one plane
template <typename TA, typename TB, bool VEC>
__global__ void __launch_bounds__(kThreads) sse_partial_kernel(const TA* __restrict__ a, const TB* __restrict__ b, int H, int W,
                                                               long long row_stride, long long plane_stride,
                                                               double* __restrict__ partial)
{
    __shared__ double scratch[kThreads / 64];
    const unsigned wv = (W + 7) >> 3;
    const unsigned pieces = static_cast<unsigned>(H) * wv;       // < 2^31 (sse_validate)
    const long long base = static_cast<long long>(blockIdx.y) * plane_stride;
    double s = 0.0;
    for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < pieces; i += gridDim.x * kThreads) {
        const int h = static_cast<int>(i / wv), w0 = static_cast<int>(i - h * wv) * 8;
        const long long off = base + h * row_stride + w0;
        if constexpr (VEC) {
            const Vec8<TA> va = load8(a + off);
            const Vec8<TB> vb = load8(b + off);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const double d = sample(va.v[e]) - sample(vb.v[e]);
                s += d * d;
            }
        } else {
            const int n = min(8, W - w0);
            for (int e = 0; e < n; ++e) {
                const double d = sample(a[off + e]) - sample(b[off + e]);
                s += d * d;
            }
        }
    }
    const double t = block_sum(s, scratch);
    if (threadIdx.x == 0) partial[static_cast<long long>(blockIdx.y) * gridDim.x + blockIdx.x] = t;
}

// out[plane] = the sum of that plane's `parts` partials, in a fixed order
__global__ void __launch_bounds__(kThreads) sse_final_kernel(const double* __restrict__ partial, int parts, double* __restrict__ out)
{
    __shared__ double scratch[kThreads / 64];
    const double* q = partial + static_cast<long long>(blockIdx.x) * parts;
    double s = 0.0;
    for (int k = threadIdx.x; k < parts; k += kThreads) s += q[k];
    const double t = block_sum(s, scratch);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

int sse_parts(int H, int W)
{
    const long long pieces = static_cast<long long>(H) * ((W + 7) / 8);
    return static_cast<int>(std::min<long long>(kSsePartials, (pieces + kThreads - 1) / kThreads));
}

template <typename TA, typename TB>
void launch_sse(const TA* a, const TB* b, const SseDesc& d, double* partial, int parts, hipStream_t stream)
{
    // 8-sample pieces: one 8-B (u8) or 16-B (fp16, u16) load, or two 16-B loads (fp32), per operand
    const bool vec = d.W % 8 == 0 && d.row_stride % 8 == 0 && (d.n_planes == 1 || d.plane_stride % 8 == 0) &&
                     aligned(a, std::min<size_t>(16, 8 * sizeof(TA))) && aligned(b, std::min<size_t>(16, 8 * sizeof(TB)));
    const dim3 grid(static_cast<unsigned>(parts), static_cast<unsigned>(d.n_planes));
    if (vec) {
        hipLaunchKernelGGL((sse_partial_kernel<TA, TB, true>), grid, dim3(kThreads), 0, stream, a, b, d.H, d.W,
                           static_cast<long long>(d.row_stride), d.plane_stride, partial);
    } else {
        hipLaunchKernelGGL((sse_partial_kernel<TA, TB, false>), grid, dim3(kThreads), 0, stream, a, b, d.H, d.W,
                           static_cast<long long>(d.row_stride), d.plane_stride, partial);
    }
}

template <typename TA>
void launch_sse_b(const TA* a, const SseDesc& d, double* partial, int parts, hipStream_t stream)
{
    switch (d.rec_dtype) {
    case kSampleU8: launch_sse(a, static_cast<const uint8_t*>(d.rec), d, partial, parts, stream); break;
    case kSampleF16: launch_sse(a, static_cast<const half_t*>(d.rec), d, partial, parts, stream); break;
    case kSampleU16: launch_sse(a, static_cast<const uint16_t*>(d.rec), d, partial, parts, stream); break;
    default: launch_sse(a, static_cast<const float*>(d.rec), d, partial, parts, stream); break;
    }
}

}  // namespace

void sse_validate(const SseDesc& d)
{
    if (d.src == nullptr || d.rec == nullptr || d.out == nullptr) throw std::invalid_argument("sse: null operand");
    for (int t : {d.src_dtype, d.rec_dtype}) {
        if (!known_sample(t)) throw std::invalid_argument("sse: unknown sample type " + std::to_string(t));
    }
    if (d.n_planes <= 0 || d.H <= 0 || d.W <= 0) throw std::invalid_argument("sse: empty geometry");
    if (d.n_planes > 65535) throw std::invalid_argument("sse: at most 65535 planes per call");
    // 32-bit piece indices: 8 samples per piece, the last workgroup's stride included
    if (static_cast<long long>(d.H) * ((d.W + 7) / 8) + static_cast<long long>(kSsePartials) * kThreads > (1LL << 31)) {
        throw std::invalid_argument("sse: plane too large");
    }
    if (d.row_stride < d.W) throw std::invalid_argument("sse: row stride below the plane width");
    if (d.n_planes > 1 && d.plane_stride < static_cast<long long>(d.H - 1) * d.row_stride + d.W) {
        throw std::invalid_argument("sse: plane stride below the plane size");
    }
}

size_t sse_workspace_bytes(int n_planes, int H, int W)
{
    return static_cast<size_t>(n_planes) * sse_parts(H, W) * sizeof(double);
}

void sse(const SseDesc& d, void* workspace, hipStream_t stream)
{
    sse_validate(d);
    double* partial = static_cast<double*>(workspace);
    const int parts = sse_parts(d.H, d.W);
    switch (d.src_dtype) {
    case kSampleU8: launch_sse_b(static_cast<const uint8_t*>(d.src), d, partial, parts, stream); break;
    case kSampleF16: launch_sse_b(static_cast<const half_t*>(d.src), d, partial, parts, stream); break;
    case kSampleU16: launch_sse_b(static_cast<const uint16_t*>(d.src), d, partial, parts, stream); break;
    default: launch_sse_b(static_cast<const float*>(d.src), d, partial, parts, stream); break;
    }
    hip_check(hipGetLastError(), "sse launch");
    hipLaunchKernelGGL(sse_final_kernel, dim3(d.n_planes), dim3(kThreads), 0, stream, partial, parts, d.out);
    hip_check(hipGetLastError(), "sse final launch");
}

}  // namespace dcvc
