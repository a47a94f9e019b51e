// scene.hip - the measurement behind scene-cut detection: the 8-bit luma plane of a picture in the codec's
// own input layout, and its sum of absolute differences against the previous picture's plane, on the GPU.
//
// x is what yuv420_to_x / yuv420p16_to_x / rgb_to_x write: fp16, pixel p = r W + c at x + p ldx, luma in channel 0 as
// value / max - 0.5. L = clamp(rintf((float(x0) + 0.5f) * 255.f), 0, 255): two fp32 operations (the library builds with
// -ffp-contract=off: no v_fma) and a round half to even; for an 8-bit source that is the source's luma sample, all 256 of
// them. NaN counts as 0.
//
// One HBM-bound pass, one thread per 8 consecutive pixels (the planes are dense, so pixels are numbered across rows).
// VEC_X: x at ldx == 3 on a 16-byte boundary, 3 x 16-B loads per thread; otherwise one 2-B load per pixel at stride ldx
// (the slots of a chunk at x + 6 j bytes, ldx = 24). VEC_L: the luma planes on 8-byte boundaries, one 8-B load and store
// per thread; otherwise bytes. The sum is an integer: per thread at most 8 x 255, per wave and workgroup in 32 bits,
// then one 64-bit atomic add per workgroup onto a sum a first, one-thread launch has zeroed. Integer addition commutes,
// so the result does not depend on the order the workgroups arrive in. Without a previous plane there is one launch and
// its first thread writes the 0.
#include "ops.h"

namespace dcvc {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ unsigned luma8_of(half_t x0)
{
    const float v = (static_cast<float>(x0) + 0.5f) * 255.f;
    const float r = rintf(v);
    return r >= 255.f ? 255u : (r > 0.f ? static_cast<unsigned>(r) : 0u);      // NaN fails both tests: 0
}

__device__ __forceinline__ unsigned absdiff(unsigned a, unsigned b) { return a > b ? a - b : b - a; }

__global__ void scene_zero_kernel(unsigned long long* __restrict__ sad) { *sad = 0ull; }

template <bool VEC_X, bool VEC_L, bool HAS_PREV>
__global__ void __launch_bounds__(kThreads) luma_sad_kernel(const half_t* __restrict__ x, long long ldx, long long pixels,
                                                            const uint8_t* __restrict__ prev, uint8_t* __restrict__ luma,
                                                            unsigned long long* __restrict__ sad)
{
    __shared__ unsigned scratch[kThreads / 64];
    const long long p0 = (static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x) * 8;
    unsigned s = 0;
    if (p0 + 8 <= pixels) {
        unsigned l[8];
        if constexpr (VEC_X) {
            // 8 pixels = 24 halfs = 3 x 16 B; luma at halfs 0, 3, ..., 21
            union { uint4 q[3]; half_t h[24]; } v;
            const uint4* src = reinterpret_cast<const uint4*>(x + p0 * 3);
            v.q[0] = src[0]; v.q[1] = src[1]; v.q[2] = src[2];
#pragma unroll
            for (int e = 0; e < 8; ++e) l[e] = luma8_of(v.h[3 * e]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) l[e] = luma8_of(x[(p0 + e) * ldx]);
        }
        if constexpr (HAS_PREV) {
            if constexpr (VEC_L) {
                const uint2 pv = *reinterpret_cast<const uint2*>(prev + p0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s += absdiff(l[e], (pv.x >> (8 * e)) & 255u);
                    s += absdiff(l[4 + e], (pv.y >> (8 * e)) & 255u);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) s += absdiff(l[e], prev[p0 + e]);
            }
        }
        if constexpr (VEC_L) {
            uint2 o;
            o.x = l[0] | (l[1] << 8) | (l[2] << 16) | (l[3] << 24);
            o.y = l[4] | (l[5] << 8) | (l[6] << 16) | (l[7] << 24);
            *reinterpret_cast<uint2*>(luma + p0) = o;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) luma[p0 + e] = static_cast<uint8_t>(l[e]);
        }
    } else {
        // the ragged end of the plane: fewer than 8 pixels, element accesses
        for (long long p = p0; p < pixels; ++p) {
            const unsigned l = luma8_of(x[p * ldx]);
            if constexpr (HAS_PREV) s += absdiff(l, prev[p]);
            luma[p] = static_cast<uint8_t>(l);
        }
    }
    if constexpr (HAS_PREV) {
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
        if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned t = 0;                                        // <= 256 x 8 x 255
            for (int k = 0; k < kThreads / 64; ++k) t += scratch[k];
            if (t) atomicAdd(sad, static_cast<unsigned long long>(t));
        }
    } else {
        if (blockIdx.x == 0 && threadIdx.x == 0) *sad = 0ull;
    }
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <bool VEC_X, bool VEC_L>
void launch(const LumaSadDesc& d, hipStream_t stream)
{
    const long long pixels = static_cast<long long>(d.H) * d.W;
    const unsigned grid = static_cast<unsigned>(((pixels + 7) / 8 + kThreads - 1) / kThreads);      // <= 2^17 (validate)
    unsigned long long* sad = static_cast<unsigned long long*>(d.sad);
    if (d.prev != nullptr) {
        hipLaunchKernelGGL(scene_zero_kernel, dim3(1), dim3(1), 0, stream, sad);
        hip_check(hipGetLastError(), "luma_sad zero launch");
        hipLaunchKernelGGL((luma_sad_kernel<VEC_X, VEC_L, true>), dim3(grid), dim3(kThreads), 0, stream, d.x,
                           static_cast<long long>(d.ldx), pixels, d.prev, d.luma, sad);
    } else {
        hipLaunchKernelGGL((luma_sad_kernel<VEC_X, VEC_L, false>), dim3(grid), dim3(kThreads), 0, stream, d.x,
                           static_cast<long long>(d.ldx), pixels, d.prev, d.luma, sad);
    }
    hip_check(hipGetLastError(), "luma_sad launch");
}

}  // namespace

void luma_sad_validate(const LumaSadDesc& d)
{
    if (d.x == nullptr || d.luma == nullptr || d.sad == nullptr) throw std::invalid_argument("luma_sad: null operand");
    if (d.H < 1 || d.W < 1 || d.ldx < 1) throw std::invalid_argument("luma_sad: H, W and ldx must be positive");
    if (d.H > kLumaSadMaxSide || d.W > kLumaSadMaxSide) {
        throw std::invalid_argument("luma_sad: picture side above " + std::to_string(kLumaSadMaxSide) + ", got " +
                                    std::to_string(d.W) + "x" + std::to_string(d.H));
    }
    if (d.luma == d.prev) throw std::invalid_argument("luma_sad: luma8_out must not be prev_luma8 (two planes, used in turn)");
    if (!aligned(d.x, 2)) throw std::invalid_argument("luma_sad: x must be 2-byte aligned");
    if (!aligned(d.sad, 8)) throw std::invalid_argument("luma_sad: sad_out must be 8-byte aligned");
}

void luma_sad(const LumaSadDesc& d, hipStream_t stream)
{
    luma_sad_validate(d);
    const bool vec_x = d.ldx == 3 && aligned(d.x, 16);
    const bool vec_l = aligned(d.luma, 8) && (d.prev == nullptr || aligned(d.prev, 8));
    if (vec_x && vec_l) launch<true, true>(d, stream);
    else if (vec_x) launch<true, false>(d, stream);
    else if (vec_l) launch<false, true>(d, stream);
    else launch<false, false>(d, stream);
}

}  // namespace dcvc
