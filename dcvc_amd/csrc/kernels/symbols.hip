// symbols.hip - the HBM-bound "symbol" kernels between the prior networks and the host rANS
// coder: masked quantisation, scale -> CDF-index mapping, skip flags, stream compaction and the
// decoder-side inverse. Reference: elementwise/stream.cu.
//
// MI355X-first re-design:
//   * one fused kernel per autoregressive step instead of the reference's 6 launches
//     (process_with_mask + 2x single_part_for_writing_4x + build_index_enc + 3 compaction steps):
//     the 4x checkerboard masks (dmci_proxy.cpp:678-699) activate exactly ONE of the four channel
//     groups at every pixel, so "multiply by the mask and fold the four groups" is a gather of the
//     active group - bit-identical results, 1/4 of the arithmetic and no mask tensors in HBM;
//   * the fp16 log of scale_to_index (stream.cu:77-87) is a table lookup on the fp16 bit pattern
//     (monotone, 7.4 K entries, built once on the host with correctly rounded fp16 steps) so
//     encoder, decoder and the CPU oracle agree bit for bit;
//   * stream compaction by wave64 ballot/popcount ranks + one 256-entry block scan (the reference
//     uses a 1024-thread shared-memory Hillis-Steele scan, stream.cu:176-282), symbols are laid
//     out NHWC exactly as stream.cu:96-97 orders them.
#include "arith.h"
#include "ops.h"

#include <cmath>
#include <mutex>
#include <vector>

namespace dcvc {

namespace {

constexpr int kElemsPerThread = 8;
constexpr int kBlockThreads = 256;
constexpr int kBlockElems = kElemsPerThread * kBlockThreads;   // 2048

// ----------------------------------------------------------------- scale -> index table
// def_const.h:6-12 evaluated in fp16 exactly as the kernel parameters of stream.cu:77-87 are:
//   idx = floor( h( h( h(log(clamp(s))) - h(LOG_SCALE_MIN) ) * h(LOG_SCALE_STEP_RECIP) ) )
constexpr float kScaleMin = 0.11f;
constexpr float kScaleMax = 16.f;
constexpr float kLogScaleMin = -2.2073f;
constexpr float kLogScaleMax = 2.7726f;
constexpr float kLogScaleStepRecip = 1.f / ((kLogScaleMax - kLogScaleMin) / 127);

uint16_t half_bits(half_t h)
{
    uint16_t b;
    __builtin_memcpy(&b, &h, 2);
    return b;
}

struct Lut {
    uint8_t* dev = nullptr;
    uint16_t lo = 0, hi = 0;     // fp16 bit patterns of the clamped range
};

Lut& lut()
{
    static Lut g;
    static std::once_flag once;
    std::call_once(once, [] {
        const half_t hmin = static_cast<half_t>(kScaleMin), hmax = static_cast<half_t>(kScaleMax);
        const half_t hlogmin = static_cast<half_t>(kLogScaleMin);
        const half_t hrecip = static_cast<half_t>(kLogScaleStepRecip);
        g.lo = half_bits(hmin);
        g.hi = half_bits(hmax);
        std::vector<uint8_t> host(static_cast<size_t>(g.hi - g.lo) + 1);
        for (uint32_t b = g.lo; b <= g.hi; ++b) {
            const uint16_t bb = static_cast<uint16_t>(b);
            half_t s;
            __builtin_memcpy(&s, &bb, 2);
            const half_t l = static_cast<half_t>(std::log(static_cast<double>(s)));
            const half_t d = static_cast<half_t>(static_cast<float>(l) - static_cast<float>(hlogmin));
            const half_t v = static_cast<half_t>(static_cast<float>(d) * static_cast<float>(hrecip));
            int idx = static_cast<int>(std::floor(static_cast<float>(v)));
            idx = idx < 0 ? 0 : (idx > 127 ? 127 : idx);
            host[b - g.lo] = static_cast<uint8_t>(idx);
        }
        hip_check(hipMalloc(&g.dev, host.size()), "hipMalloc(scale lut)");
        hip_check(hipMemcpy(g.dev, host.data(), host.size(), hipMemcpyHostToDevice), "upload scale lut");
    });
    return g;
}

struct LutView {
    const uint8_t* tab;
    uint16_t lo, hi;
};

__device__ __forceinline__ int scale_to_index(half_t s, const LutView& v)
{
    uint16_t b;
    __builtin_memcpy(&b, &s, 2);
    // clamp on the value (negative / tiny / NaN scales go to the first entry, like max(s, min))
    if (!(static_cast<float>(s) > 0.f)) {
        b = v.lo;
    }
    b = b < v.lo ? v.lo : (b > v.hi ? v.hi : b);   // positive fp16 bit patterns order like values
    return v.tab[b - v.lo];
}

__device__ __forceinline__ int active_group(int step, int h, int w)
{
    const int pos = ((h & 1) << 1) | (w & 1);
    // mask_k = cat over groups of micro masks, common_model.py:174-195 / dmci_proxy.cpp:678-699
    return step == 0 ? pos : step == 1 ? 3 - pos : step == 2 ? (pos ^ 2) : (pos ^ 1);
}

__device__ __forceinline__ int block_sum_256(int v, int* lds)
{
    // returns the sum over the block in every thread (4 waves)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[wave] = v;
    __syncthreads();
    const int s = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return s;
}

// ----------------------------------------------------------------- batches
// A batch of pictures runs as a 2-D grid: blockIdx.x = the 2048-element block inside the picture, blockIdx.y = the picture.
// Each picture's operands start at its own offset, so every block sees exactly what it sees in a single launch: the masks
// follow the picture's own (y, x), block counts and compaction regions are the picture's own.
__device__ __forceinline__ size_t pic_pixels(int H, int W)
{
    return static_cast<size_t>(blockIdx.y) * H * W;
}

__device__ __forceinline__ YStepEnc at_picture(const YStepEnc& d)
{
    YStepEnc e = d;
    const size_t pix = pic_pixels(d.H, d.W), sym = pix * (d.C >> 2);
    e.y += pix * d.ldy; e.scales += pix * d.lds; e.means += pix * d.ldm; e.y_hat_acc += pix * d.ldacc;
    e.sym += sym; e.cond += sym >> 3; e.block_count += static_cast<size_t>(blockIdx.y) * gridDim.x;
    return e;
}

__device__ __forceinline__ YStepDecIndex at_picture(const YStepDecIndex& d)
{
    YStepDecIndex e = d;
    const size_t pix = pic_pixels(d.H, d.W), sym = pix * (d.C >> 2);
    e.scales += pix * d.lds;
    e.index += sym; e.cond += sym >> 3; e.block_count += static_cast<size_t>(blockIdx.y) * gridDim.x;
    return e;
}

__device__ __forceinline__ YStepDecRestore at_picture(const YStepDecRestore& d)
{
    YStepDecRestore e = d;
    const size_t pix = pic_pixels(d.H, d.W), sym = pix * (d.C >> 2);
    e.decoded += blockIdx.y * d.decoded_stride; e.totals += static_cast<size_t>(blockIdx.y) * d.totals_stride;
    e.cond += sym >> 3; e.block_count += static_cast<size_t>(blockIdx.y) * gridDim.x;
    e.means += pix * d.ldm; e.y_hat_acc += pix * d.ldacc;
    return e;
}

// ----------------------------------------------------------------- encoder step
__global__ void __launch_bounds__(kBlockThreads)
y_step_enc_kernel(const YStepEnc dk, const LutView lutv, const half_t thres)
{
    const YStepEnc d = at_picture(dk);
    __shared__ int lds[4];
    const int cq = d.C >> 2;
    const int total = d.H * d.W * cq;
    const int e0 = (blockIdx.x * kBlockThreads + threadIdx.x) * kElemsPerThread;
    int kept = 0;
    if (e0 < total) {
        const int pix = e0 / cq;
        const int c = e0 - pix * cq;
        const int h = pix / d.W, w = pix - h * d.W;
        const int g = active_group(d.step, h, w);
        const int ch = g * cq + c;
        const half8 y8 = *reinterpret_cast<const half8*>(d.y + static_cast<size_t>(pix) * d.ldy + ch);
        const half8 s8 = *reinterpret_cast<const half8*>(d.scales + static_cast<size_t>(pix) * d.lds + ch);
        const half8 m8 = *reinterpret_cast<const half8*>(d.means + static_cast<size_t>(pix) * d.ldm + ch);
        half8 yh;
        short sym[8];
        unsigned flags = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            // process_with_mask_kernel, stream.cu:549-630 (active lanes of the mask)
            const half_t y_res = hsub(y8[i], m8[i]);
            float q = round_half_away(static_cast<float>(y_res));
            const bool keep = static_cast<float>(s8[i]) > static_cast<float>(thres);
            q = keep ? q : 0.f;
            q = fmaxf(fminf(q, 127.f), -128.f);
            yh[i] = to_half(q + static_cast<float>(m8[i]));
            // build_index_enc_kernel, stream.cu:130-161
            const int idx = scale_to_index(s8[i], lutv);
            sym[i] = static_cast<short>(static_cast<int>(q) * 256 + idx);
            flags |= (keep ? 1u : 0u) << i;
        }
        half_t* acc = d.y_hat_acc + static_cast<size_t>(pix) * d.ldacc;
        *reinterpret_cast<half8*>(acc + ch) = yh;
        if (d.first) {
            const half8 zero = { 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
            for (int og = 1; og < 4; ++og) {
                *reinterpret_cast<half8*>(acc + ((g + og) & 3) * cq + c) = zero;
            }
        }
        typedef short short8 __attribute__((ext_vector_type(8)));
        short8 s_out;
#pragma unroll
        for (int i = 0; i < 8; ++i) s_out[i] = sym[i];
        *reinterpret_cast<short8*>(d.sym + e0) = s_out;
        d.cond[e0 >> 3] = static_cast<uint8_t>(flags);
        kept = __popc(flags);
    }
    const int s = block_sum_256(kept, lds);
    if (threadIdx.x == 0) d.block_count[blockIdx.x] = s;
}

// ----------------------------------------------------------------- decoder index step
__global__ void __launch_bounds__(kBlockThreads)
y_step_dec_index_kernel(const YStepDecIndex dk, const LutView lutv, const half_t thres)
{
    const YStepDecIndex d = at_picture(dk);
    __shared__ int lds[4];
    const int cq = d.C >> 2;
    const int total = d.H * d.W * cq;
    const int e0 = (blockIdx.x * kBlockThreads + threadIdx.x) * kElemsPerThread;
    int kept = 0;
    if (e0 < total) {
        const int pix = e0 / cq;
        const int c = e0 - pix * cq;
        const int h = pix / d.W, w = pix - h * d.W;
        const int ch = active_group(d.step, h, w) * cq + c;
        const half8 s8 = *reinterpret_cast<const half8*>(d.scales + static_cast<size_t>(pix) * d.lds + ch);
        unsigned flags = 0;
        typedef unsigned char uchar8 __attribute__((ext_vector_type(8)));
        uchar8 idx8;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            idx8[i] = static_cast<unsigned char>(scale_to_index(s8[i], lutv));
            flags |= (static_cast<float>(s8[i]) > static_cast<float>(thres) ? 1u : 0u) << i;
        }
        *reinterpret_cast<uchar8*>(d.index + e0) = idx8;
        d.cond[e0 >> 3] = static_cast<uint8_t>(flags);
        kept = __popc(flags);
    }
    const int s = block_sum_256(kept, lds);
    if (threadIdx.x == 0) d.block_count[blockIdx.x] = s;
}

// ----------------------------------------------------------------- compaction / recovery
// exclusive rank of this thread's first kept element inside the block + the block base
__device__ __forceinline__ int block_base_and_rank(const int32_t* block_count, const int32_t* totals,
                                                   int slot, int kept, int* lds, int& step_base)
{
    // sum of the counts of all earlier blocks (<= a few hundred blocks: one strided pass)
    int part = 0;
    for (int b = threadIdx.x; b < static_cast<int>(blockIdx.x); b += kBlockThreads) part += block_count[b];
    const int before = block_sum_256(part, lds);
    // prefix inside the block: wave scan + 4 wave totals
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = kept;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    int wave_off = 0;
    for (int i = 0; i < wave; ++i) wave_off += lds[i];
    __syncthreads();
    step_base = 0;
    for (int i = 0; i < slot; ++i) step_base += totals[i];
    return step_base + before + wave_off + incl - kept;
}

template <typename T>
__global__ void __launch_bounds__(kBlockThreads)
compact_kernel(const T* __restrict__ in, const uint8_t* __restrict__ cond,
               const int32_t* __restrict__ block_count, int count, T* __restrict__ out,
               int32_t* totals, int slot, long long out_stride, int totals_stride)
{
    // a batch (blockIdx.y = picture): each picture of `count` elements into its own region
    in += static_cast<size_t>(blockIdx.y) * count;
    cond += (static_cast<size_t>(blockIdx.y) * count) >> 3;
    block_count += static_cast<size_t>(blockIdx.y) * gridDim.x;
    out += blockIdx.y * out_stride;
    totals += static_cast<size_t>(blockIdx.y) * totals_stride;
    __shared__ int lds[4];
    const int e0 = (blockIdx.x * kBlockThreads + threadIdx.x) * kElemsPerThread;
    unsigned flags = 0;
    if (e0 < count) flags = cond[e0 >> 3];
    int step_base;
    int pos = block_base_and_rank(block_count, totals, slot, __popc(flags), lds, step_base);
    if (flags) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (flags & (1u << i)) out[pos++] = in[e0 + i];
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == kBlockThreads - 1) {
        totals[slot] = pos - step_base;   // everything kept lies before the last thread's end
    }
}

__global__ void __launch_bounds__(kBlockThreads)
y_step_dec_restore_kernel(const YStepDecRestore dk)
{
    const YStepDecRestore d = at_picture(dk);
    __shared__ int lds[4];
    const int cq = d.C >> 2;
    const int total = d.H * d.W * cq;
    const int e0 = (blockIdx.x * kBlockThreads + threadIdx.x) * kElemsPerThread;
    unsigned flags = 0;
    if (e0 < total) flags = d.cond[e0 >> 3];
    int step_base;
    int pos = block_base_and_rank(d.block_count, d.totals, d.slot, __popc(flags), lds, step_base);
    if (e0 >= total) return;
    const int pix = e0 / cq;
    const int c = e0 - pix * cq;
    const int h = pix / d.W, w = pix - h * d.W;
    const int g = active_group(d.step, h, w);
    const int ch = g * cq + c;
    const half8 m8 = *reinterpret_cast<const half8*>(d.means + static_cast<size_t>(pix) * d.ldm + ch);
    half8 yh;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        // conditional_recover (stream.cu:360-383) + restore_y_4x (stream.cu:757-792)
        float q = 0.f;
        if (flags & (1u << i)) q = static_cast<float>(d.decoded[pos++]);
        yh[i] = to_half(q + static_cast<float>(m8[i]));
    }
    half_t* acc = d.y_hat_acc + static_cast<size_t>(pix) * d.ldacc;
    *reinterpret_cast<half8*>(acc + ch) = yh;
    if (d.first) {
        const half8 zero = { 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
        for (int og = 1; og < 4; ++og) {
            *reinterpret_cast<half8*>(acc + ((g + og) & 3) * cq + c) = zero;
        }
    }
}

// ----------------------------------------------------------------- full-tensor masked steps (inter models)
// the step in which channel `ch` of pixel (h, w) is coded
__device__ __forceinline__ int step_of(int nsteps, int h, int w, int ch, int C)
{
    if (nsteps == 2) {
        const bool even = ((h ^ w) & 1) == 0;
        const bool first = ch < (C >> 1);
        return even == first ? 0 : 1;
    }
    const int g = ch / (C >> 2);
    const int pos = ((h & 1) << 1) | (w & 1);
    return g == pos ? 0 : g == 3 - pos ? 1 : g == (pos ^ 2) ? 2 : 3;     // inverse of active_group()
}

__device__ __forceinline__ half_t clamp_min_half(half_t q)
{
    return static_cast<float>(q) > 0.5f ? q : static_cast<half_t>(0.5f);     // max(q, 0.5); NaN -> 0.5
}

__global__ void __launch_bounds__(kBlockThreads)
mask_step_enc_kernel(const MaskStepEnc d, const LutView lutv, const half_t thres)
{
    __shared__ int lds[4];
    const int total = d.H * d.W * d.C;
    const int e0 = (blockIdx.x * kBlockThreads + threadIdx.x) * kElemsPerThread;
    const bool first = d.step == 0, last = d.step == d.nsteps - 1;
    int kept = 0;
    if (e0 < total) {
        const int pix = e0 / d.C;
        const int ch = e0 - pix * d.C;
        const int h = pix / d.W, w = pix - h * d.W;
        const bool active = step_of(d.nsteps, h, w, ch, d.C) == d.step;
        if (active || first || last) {
            half_t* yp = d.y + static_cast<size_t>(pix) * d.ldy + ch;
            half_t* yhp = d.y_hat + static_cast<size_t>(pix) * d.ldh + ch;
            const half8 q8 = *reinterpret_cast<const half8*>(d.q_dec + static_cast<size_t>(pix) * d.ldq + ch);
            const half8 s8 = *reinterpret_cast<const half8*>(d.scales + static_cast<size_t>(pix) * d.lds + ch);
            half8 y8 = *reinterpret_cast<const half8*>(yp);
            if (first) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const half_t r = to_half(1.0f / static_cast<float>(clamp_min_half(q8[i])));
                    y8[i] = hmul(y8[i], r);
                }
                *reinterpret_cast<half8*>(yp) = y8;
            }
            half8 yh = { 0, 0, 0, 0, 0, 0, 0, 0 };
            if (active) {
                const half8 m8 = *reinterpret_cast<const half8*>(d.means + static_cast<size_t>(pix) * d.ldm + ch);
                typedef short short8 __attribute__((ext_vector_type(8)));
                short8 s_out;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const half_t y_res = hsub(y8[i], m8[i]);
                    float q = round_half_away(static_cast<float>(y_res));
                    const bool keep = static_cast<float>(s8[i]) > static_cast<float>(thres);
                    q = keep ? q : 0.f;
                    q = fmaxf(fminf(q, 127.f), -128.f);
                    yh[i] = to_half(q + static_cast<float>(m8[i]));
                    s_out[i] = static_cast<short>(static_cast<int>(q) * 256 + scale_to_index(s8[i], lutv));
                }
                *reinterpret_cast<short8*>(d.sym + e0) = s_out;
            } else if (!first) {
                yh = *reinterpret_cast<const half8*>(yhp);       // an earlier step's result (last step only)
            }
            if (last) {
                unsigned flags = 0;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    yh[i] = hmul(yh[i], clamp_min_half(q8[i]));
                    flags |= (static_cast<float>(s8[i]) > static_cast<float>(thres) ? 1u : 0u) << i;
                }
                d.cond[e0 >> 3] = static_cast<uint8_t>(flags);
                kept = __popc(flags);
            }
            *reinterpret_cast<half8*>(yhp) = yh;
        }
    }
    if (last) {
        const int s = block_sum_256(kept, lds);
        if (threadIdx.x == 0) d.block_count[blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(kBlockThreads)
mask_dec_index_kernel(const MaskDecIndex d, const LutView lutv, const half_t thres)
{
    __shared__ int lds[4];
    const int total = d.H * d.W * d.C;
    const int e0 = (blockIdx.x * kBlockThreads + threadIdx.x) * kElemsPerThread;
    int kept = 0;
    if (e0 < total) {
        const int pix = e0 / d.C;
        const int ch = e0 - pix * d.C;
        const half8 s8 = *reinterpret_cast<const half8*>(d.scales + static_cast<size_t>(pix) * d.lds + ch);
        unsigned flags = 0;
        typedef unsigned char uchar8 __attribute__((ext_vector_type(8)));
        uchar8 idx8;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            idx8[i] = static_cast<unsigned char>(scale_to_index(s8[i], lutv));
            flags |= (static_cast<float>(s8[i]) > static_cast<float>(thres) ? 1u : 0u) << i;
        }
        *reinterpret_cast<uchar8*>(d.index + e0) = idx8;
        d.cond[e0 >> 3] = static_cast<uint8_t>(flags);
        kept = __popc(flags);
    }
    const int s = block_sum_256(kept, lds);
    if (threadIdx.x == 0) d.block_count[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kBlockThreads)
mask_step_dec_kernel(const MaskStepDec d)
{
    __shared__ int lds[4];
    const int total = d.H * d.W * d.C;
    const int e0 = (blockIdx.x * kBlockThreads + threadIdx.x) * kElemsPerThread;
    const bool first = d.step == 0, last = d.step == d.nsteps - 1;
    typedef signed char char8 __attribute__((ext_vector_type(8)));
    char8 q8 = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (first) {
        unsigned flags = 0;
        if (e0 < total) flags = d.cond[e0 >> 3];
        int step_base;
        int pos = block_base_and_rank(d.block_count, d.totals, 0, __popc(flags), lds, step_base);
        if (e0 >= total) return;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (flags & (1u << i)) q8[i] = d.decoded[pos++];
        }
    }
    if (e0 >= total) return;
    const int pix = e0 / d.C;
    const int ch = e0 - pix * d.C;
    const int h = pix / d.W, w = pix - h * d.W;
    const bool active = step_of(d.nsteps, h, w, ch, d.C) == d.step;
    if (!(active || first || last)) return;
    half_t* yhp = d.y_hat + static_cast<size_t>(pix) * d.ldh + ch;
    half8 yh = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (active) {
        if (!first) q8 = *reinterpret_cast<const char8*>(d.yq + e0);
        const half8 m8 = *reinterpret_cast<const half8*>(d.means + static_cast<size_t>(pix) * d.ldm + ch);
#pragma unroll
        for (int i = 0; i < 8; ++i) yh[i] = to_half(static_cast<float>(q8[i]) + static_cast<float>(m8[i]));
    } else if (first) {
        *reinterpret_cast<char8*>(d.yq + e0) = q8;
    } else {
        yh = *reinterpret_cast<const half8*>(yhp);
    }
    if (last) {
        const half8 qd = *reinterpret_cast<const half8*>(d.q_dec + static_cast<size_t>(pix) * d.ldq + ch);
#pragma unroll
        for (int i = 0; i < 8; ++i) yh[i] = hmul(yh[i], clamp_min_half(qd[i]));
    }
    *reinterpret_cast<half8*>(yhp) = yh;
}

// ----------------------------------------------------------------- z
__global__ void round_z_kernel(const half_t* __restrict__ z, half_t* __restrict__ z_hat,
                               int8_t* __restrict__ z_i8, int count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) {
        // round_z_kernel, stream.cu:862-884: round half away, clamp to [-64, 63]
        float v = round_half_away(static_cast<float>(z[i]));
        v = fminf(fmaxf(v, -64.f), 63.f);
        z_hat[i] = to_half(v);
        z_i8[i] = static_cast<int8_t>(v);
    }
}

__global__ void int8_to_half_kernel(const int8_t* __restrict__ in, half_t* __restrict__ out, int count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = static_cast<half_t>(static_cast<float>(in[i]));
}

LutView lut_view()
{
    Lut& l = lut();
    return LutView{ l.dev, l.lo, l.hi };
}

int grid_for(int count)
{
    return (count + kBlockElems - 1) / kBlockElems;
}

void check_pictures(int n, const char* what)
{
    if (n < 1 || n > 65535) throw std::invalid_argument(std::string(what) + ": batch size out of range");
}

}  // namespace

void symbols_init()
{
    (void)lut();
}

int symbol_blocks(int count)
{
    return grid_for(count);
}

void y_step_enc(const YStepEnc& d, hipStream_t stream)
{
    if (d.C % 32 != 0) throw std::invalid_argument("y_step_enc: C must be a multiple of 32");
    check_pictures(d.n, "y_step_enc");
    const int count = d.H * d.W * (d.C / 4);
    hipLaunchKernelGGL(y_step_enc_kernel, dim3(grid_for(count), d.n), dim3(kBlockThreads), 0, stream, d,
                       lut_view(), static_cast<half_t>(d.skip_thres));
    hip_check(hipGetLastError(), "y_step_enc launch");
}

void y_step_dec_index(const YStepDecIndex& d, hipStream_t stream)
{
    if (d.C % 32 != 0) throw std::invalid_argument("y_step_dec_index: C must be a multiple of 32");
    check_pictures(d.n, "y_step_dec_index");
    const int count = d.H * d.W * (d.C / 4);
    hipLaunchKernelGGL(y_step_dec_index_kernel, dim3(grid_for(count), d.n), dim3(kBlockThreads), 0, stream,
                       d, lut_view(), static_cast<half_t>(d.skip_thres));
    hip_check(hipGetLastError(), "y_step_dec_index launch");
}

void compact(const void* in, int elem_bytes, const uint8_t* cond, const int32_t* block_count,
             int count, void* out, int32_t* totals, int slot, hipStream_t stream)
{
    compact_b(in, elem_bytes, cond, block_count, count, out, 0, totals, 0, slot, 1, stream);
}

void compact_b(const void* in, int elem_bytes, const uint8_t* cond, const int32_t* block_count, int count, void* out,
               long long out_stride, int32_t* totals, int totals_stride, int slot, int n, hipStream_t stream)
{
    check_pictures(n, "compact");
    if (n > 1 && count % 8 != 0) throw std::invalid_argument("compact: a batch needs a multiple of 8 elements per picture");
    const dim3 grid(grid_for(count), n), block(kBlockThreads);
    if (elem_bytes == 2) {
        hipLaunchKernelGGL(compact_kernel<int16_t>, grid, block, 0, stream,
                           static_cast<const int16_t*>(in), cond, block_count, count,
                           static_cast<int16_t*>(out), totals, slot, out_stride, totals_stride);
    } else if (elem_bytes == 1) {
        hipLaunchKernelGGL(compact_kernel<uint8_t>, grid, block, 0, stream,
                           static_cast<const uint8_t*>(in), cond, block_count, count,
                           static_cast<uint8_t*>(out), totals, slot, out_stride, totals_stride);
    } else {
        throw std::invalid_argument("compact: element size must be 1 or 2 bytes");
    }
    hip_check(hipGetLastError(), "compact launch");
}

void y_step_dec_restore(const YStepDecRestore& d, hipStream_t stream)
{
    if (d.C % 32 != 0) throw std::invalid_argument("y_step_dec_restore: C must be a multiple of 32");
    check_pictures(d.n, "y_step_dec_restore");
    const int count = d.H * d.W * (d.C / 4);
    hipLaunchKernelGGL(y_step_dec_restore_kernel, dim3(grid_for(count), d.n), dim3(kBlockThreads), 0,
                       stream, d);
    hip_check(hipGetLastError(), "y_step_dec_restore launch");
}

namespace {

void check_mask_steps(int C, int nsteps, int step, const char* who)
{
    if ((nsteps != 2 && nsteps != 4) || step < 0 || step >= nsteps || C % (8 * nsteps) != 0) {
        throw std::invalid_argument(std::string(who) + ": bad C / nsteps / step");
    }
}

}  // namespace

void mask_step_enc(const MaskStepEnc& d, hipStream_t stream)
{
    check_mask_steps(d.C, d.nsteps, d.step, "mask_step_enc");
    const int count = d.H * d.W * d.C;
    hipLaunchKernelGGL(mask_step_enc_kernel, dim3(grid_for(count)), dim3(kBlockThreads), 0, stream, d,
                       lut_view(), static_cast<half_t>(d.skip_thres));
    hip_check(hipGetLastError(), "mask_step_enc launch");
}

void mask_dec_index(const MaskDecIndex& d, hipStream_t stream)
{
    if (d.C % 8 != 0) throw std::invalid_argument("mask_dec_index: C must be a multiple of 8");
    const int count = d.H * d.W * d.C;
    hipLaunchKernelGGL(mask_dec_index_kernel, dim3(grid_for(count)), dim3(kBlockThreads), 0, stream, d,
                       lut_view(), static_cast<half_t>(d.skip_thres));
    hip_check(hipGetLastError(), "mask_dec_index launch");
}

void mask_step_dec(const MaskStepDec& d, hipStream_t stream)
{
    check_mask_steps(d.C, d.nsteps, d.step, "mask_step_dec");
    const int count = d.H * d.W * d.C;
    hipLaunchKernelGGL(mask_step_dec_kernel, dim3(grid_for(count)), dim3(kBlockThreads), 0, stream, d);
    hip_check(hipGetLastError(), "mask_step_dec launch");
}

void round_z(const half_t* z, half_t* z_hat, int8_t* z_i8, int count, hipStream_t stream)
{
    hipLaunchKernelGGL(round_z_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, z, z_hat, z_i8, count);
    hip_check(hipGetLastError(), "round_z launch");
}

void int8_to_half(const int8_t* in, half_t* out, int count, hipStream_t stream)
{
    hipLaunchKernelGGL(int8_to_half_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, in, out, count);
    hip_check(hipGetLastError(), "int8_to_half launch");
}

}  // namespace dcvc
