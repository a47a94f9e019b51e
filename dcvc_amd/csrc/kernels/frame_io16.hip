// frame_io16.hip - high-bit-depth (9..16 bit) YUV420 planes <-> the codec's fp16 NHWC picture tensor, on the GPU.
//
// Files of this kind (yuv420p10le and its relatives) hold uint16 little-endian samples. DCVC-FM's YUVReader /
// YUVWriter (video_reader.py:130-183, video_writer.py:86-130) define the scale: the reader computes fp32(v) / max_val with
// max_val = 2^b - 1, the writer stores clip(rint(v * max_val), 0, max_val). Here:
//   yuv420p16_to_x: d = fp16(fp32(v) / fp32(max_val)) with a correctly rounded fp32 division (the library builds with
//                   -fno-fast-math), x = fp16(fp32(d) - 0.5): frame_io.hip's load_pixel with 255 replaced by max_val;
//                   nearest-neighbour chroma. Samples above max_val are neither masked nor checked, as in FM.
//   x_to_yuv420p16: t as x_to_yuv420 computes it before its * 255 (Y: hadd(x, 0.5); U / V: fp16 x + 0.5 summed over the
//                   2 x 2 block in fp32, fp16(sum * 0.25)), then dist = clamp(fp32(t) * fp32(max_val), 0, max_val) in fp32
//                   (fp16 cannot hold a 10-bit sample to better than 0.5) and the writer's sample rint(dist), half to even,
//                   for all three planes.
// HBM-bound passes, one thread per 8 luma pixels of a row (yuv420p16_to_x) or per 8 x 2 luma pixels (x_to_yuv420p16),
// with 16-B accesses where the row allows them (W % 8 == 0, aligned bases; x at ldx == 3 / row_pixels % 8 == 0) and
// element accesses elsewhere (chunk slots at ldx = 24, widths that are no multiple of 8).
#include "arith.h"
#include "ops.h"

namespace dcvc {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ half_t load_sample(unsigned v, float maxv)
{
    const half_t d = to_half(static_cast<float>(v) / maxv);        // true division, correctly rounded
    return to_half(static_cast<float>(d) - 0.5f);
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// one thread = 8 consecutive luma pixels of a row (4 chroma samples). VEC: W % 8 == 0, 16-B aligned planes and x at
// ldx == 3: one 16-B load of Y, one 8-B load each of U and V, 3 x 16-B stores.
template <bool VEC>
__global__ void __launch_bounds__(kThreads) yuv420p16_to_x_kernel(const uint16_t* __restrict__ yp, const uint16_t* __restrict__ uvp,
                                                                  int H, int W, float maxv, half_t* __restrict__ x, int ldx)
{
    const unsigned wv = (W + 7) >> 3;
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;      // < 2^31 (validate)
    if (i >= static_cast<unsigned>(H) * wv) return;
    const int h = static_cast<int>(i / wv), w0 = static_cast<int>(i - h * wv) * 8;
    const int Hc = H >> 1, Wc = W >> 1;
    const uint16_t* yr = yp + static_cast<size_t>(h) * W + w0;
    const uint16_t* ur = uvp + static_cast<size_t>(h >> 1) * Wc;
    const uint16_t* vr = ur + static_cast<size_t>(Hc) * Wc;
    half_t* o = x + (static_cast<size_t>(h) * W + w0) * ldx;
    if constexpr (VEC) {
        const uint4 yv = *reinterpret_cast<const uint4*>(yr);
        const uint2 uv = *reinterpret_cast<const uint2*>(ur + (w0 >> 1));
        const uint2 vv = *reinterpret_cast<const uint2*>(vr + (w0 >> 1));
        const uint16_t* ys = reinterpret_cast<const uint16_t*>(&yv);
        const uint16_t* us = reinterpret_cast<const uint16_t*>(&uv);
        const uint16_t* vs = reinterpret_cast<const uint16_t*>(&vv);
        half8 out[3];
        half_t* ho = reinterpret_cast<half_t*>(out);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            ho[3 * e + 0] = load_sample(ys[e], maxv);
            ho[3 * e + 1] = load_sample(us[e >> 1], maxv);
            ho[3 * e + 2] = load_sample(vs[e >> 1], maxv);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) reinterpret_cast<half8*>(o)[k] = out[k];
    } else {
        const int n = min(8, W - w0);
        for (int e = 0; e < n; ++e) {
            const int wc = (w0 + e) >> 1;
            o[e * ldx + 0] = load_sample(yr[e], maxv);
            o[e * ldx + 1] = load_sample(ur[wc], maxv);
            o[e * ldx + 2] = load_sample(vr[wc], maxv);
        }
    }
}

// fp32 distortion sample and the writer's sample of one fp16 t in 0..1
__device__ __forceinline__ float dist_of(half_t t, float maxv)
{
    return fminf(fmaxf(static_cast<float>(t) * maxv, 0.f), maxv);
}

__device__ __forceinline__ uint16_t u16_of(float d) { return static_cast<uint16_t>(rintf(d)); }    // half to even

// one thread = 4 chroma samples = 8 x 2 luma pixels. VEC: W % 8 == 0, row_pixels % 8 == 0 and aligned bases: 3 x 16-B loads
// per luma row, 16-B (u16) / 2 x 16-B (fp32) stores per luma row, 8-B / 16-B stores per chroma plane.
template <bool VEC>
__global__ void __launch_bounds__(kThreads) x_to_yuv420p16_kernel(const half_t* __restrict__ x, int row_pixels, int H, int W,
                                                                  float maxv, float* __restrict__ dist, uint16_t* __restrict__ yuv)
{
    const int Hc = H >> 1, Wc = W >> 1;
    const unsigned wv = (Wc + 3) >> 2;
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;      // < 2^31 (validate)
    if (i >= static_cast<unsigned>(Hc) * wv) return;
    const int hc = static_cast<int>(i / wv), c0 = static_cast<int>(i - hc * wv) * 4;
    const int nc = min(4, Wc - c0);
    const size_t plane = static_cast<size_t>(H) * W, cplane = static_cast<size_t>(Hc) * Wc;
    float su[4] = {0.f, 0.f, 0.f, 0.f}, sv[4] = {0.f, 0.f, 0.f, 0.f};
    // the 2 x 2 block is summed in the order (0, 0), (0, 1), (1, 0), (1, 1), as x_to_yuv420 does
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int h = 2 * hc + dy;
        const half_t* p = x + (static_cast<size_t>(h) * row_pixels + 2 * c0) * 3;
        half_t px[24];
        if constexpr (VEC) {
#pragma unroll
            for (int k = 0; k < 3; ++k) reinterpret_cast<half8*>(px)[k] = reinterpret_cast<const half8*>(p)[k];
        } else {
            for (int e = 0; e < 2 * nc * 3; ++e) px[e] = p[e];
        }
        float dy_[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (!VEC && e >= 2 * nc) break;
            dy_[e] = dist_of(hadd(px[3 * e], static_cast<half_t>(0.5f)), maxv);           // x_hat + 0.5
            su[e >> 1] += static_cast<float>(hadd(px[3 * e + 1], static_cast<half_t>(0.5f)));
            sv[e >> 1] += static_cast<float>(hadd(px[3 * e + 2], static_cast<half_t>(0.5f)));
        }
        const size_t o = static_cast<size_t>(h) * W + 2 * c0;
        if constexpr (VEC) {
            if (dist) {
                reinterpret_cast<float4*>(dist + o)[0] = make_float4(dy_[0], dy_[1], dy_[2], dy_[3]);
                reinterpret_cast<float4*>(dist + o)[1] = make_float4(dy_[4], dy_[5], dy_[6], dy_[7]);
            }
            if (yuv) {
                uint16_t s[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) s[e] = u16_of(dy_[e]);
                *reinterpret_cast<uint4*>(yuv + o) = *reinterpret_cast<const uint4*>(s);
            }
        } else {
            for (int e = 0; e < 2 * nc; ++e) {
                if (dist) dist[o + e] = dy_[e];
                if (yuv) yuv[o + e] = u16_of(dy_[e]);
            }
        }
    }
    // avg_pool2d accumulates in fp32 and rounds once
    float du[4], dv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        du[k] = dist_of(to_half(su[k] * 0.25f), maxv);
        dv[k] = dist_of(to_half(sv[k] * 0.25f), maxv);
    }
    const size_t oc = plane + static_cast<size_t>(hc) * Wc + c0;
    if constexpr (VEC) {
        if (dist) {
            *reinterpret_cast<float4*>(dist + oc) = make_float4(du[0], du[1], du[2], du[3]);
            *reinterpret_cast<float4*>(dist + oc + cplane) = make_float4(dv[0], dv[1], dv[2], dv[3]);
        }
        if (yuv) {
            uint16_t s[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) { s[k] = u16_of(du[k]); s[4 + k] = u16_of(dv[k]); }
            *reinterpret_cast<uint2*>(yuv + oc) = reinterpret_cast<const uint2*>(s)[0];
            *reinterpret_cast<uint2*>(yuv + oc + cplane) = reinterpret_cast<const uint2*>(s)[1];
        }
    } else {
        for (int k = 0; k < nc; ++k) {
            if (dist) { dist[oc + k] = du[k]; dist[oc + cplane + k] = dv[k]; }
            if (yuv) { yuv[oc + k] = u16_of(du[k]); yuv[oc + cplane + k] = u16_of(dv[k]); }
        }
    }
}

void validate(int H, int W, int bit_depth, const char* what)
{
    if (bit_depth < 9 || bit_depth > 16) {
        throw std::invalid_argument(std::string(what) + ": bit depth must be 9..16, got " + std::to_string(bit_depth));
    }
    if (H <= 0 || W <= 0 || (H & 1) || (W & 1)) {
        throw std::invalid_argument(std::string(what) + ": the picture sides must be positive and even, got " +
                                    std::to_string(W) + "x" + std::to_string(H));
    }
    // one thread per 8 pixels of a row, 32-bit thread indices (addresses are 64-bit)
    if (static_cast<long long>(H) * ((W + 7) / 8) + kThreads > (1LL << 31)) throw std::invalid_argument(std::string(what) + ": picture too large");
}

float max_val(int bit_depth) { return static_cast<float>((1 << bit_depth) - 1); }      // exact in fp32 up to 16 bits

}  // namespace

void yuv420p16_to_x(const uint16_t* y, const uint16_t* uv, int H, int W, int bit_depth, half_t* x, int ldx, hipStream_t stream)
{
    validate(H, W, bit_depth, "yuv420p16_to_x");
    if (y == nullptr || uv == nullptr || x == nullptr) throw std::invalid_argument("yuv420p16_to_x: null operand");
    if (ldx < 3) throw std::invalid_argument("yuv420p16_to_x: the pixel stride of x must be >= 3");
    // 16-B Y rows and 8-B chroma pieces: W % 8 == 0 keeps every row start 16-B (Y) / 8-B (U, V) aligned behind an aligned base
    const bool vec = W % 8 == 0 && ldx == 3 && aligned(y, 16) && aligned(uv, 8) && aligned(x, 16);
    const long long n = static_cast<long long>(H) * ((W + 7) / 8);
    const dim3 grid(static_cast<unsigned>((n + kThreads - 1) / kThreads)), block(kThreads);
    if (vec) hipLaunchKernelGGL(yuv420p16_to_x_kernel<true>, grid, block, 0, stream, y, uv, H, W, max_val(bit_depth), x, ldx);
    else hipLaunchKernelGGL(yuv420p16_to_x_kernel<false>, grid, block, 0, stream, y, uv, H, W, max_val(bit_depth), x, ldx);
    hip_check(hipGetLastError(), "yuv420p16_to_x launch");
}

void x_to_yuv420p16(const half_t* x, int row_pixels, int H, int W, int bit_depth, float* dist, uint16_t* yuv, hipStream_t stream)
{
    validate(H, W, bit_depth, "x_to_yuv420p16");
    if (x == nullptr) throw std::invalid_argument("x_to_yuv420p16: no x_hat");
    if (row_pixels < W) throw std::invalid_argument("x_to_yuv420p16: the rows of x_hat are shorter than the picture");
    if (dist == nullptr && yuv == nullptr) return;
    // W % 8 == 0 makes Wc % 4 == 0: every chroma row starts on a 16-B (fp32) / 8-B (u16) boundary, and H W % 8 == 0 puts
    // the chroma planes behind the luma plane on those boundaries too
    const bool vec = W % 8 == 0 && row_pixels % 8 == 0 && aligned(x, 16) && (dist == nullptr || aligned(dist, 16)) &&
                     (yuv == nullptr || aligned(yuv, 16));
    const long long n = static_cast<long long>(H / 2) * ((W / 2 + 3) / 4);
    const dim3 grid(static_cast<unsigned>((n + kThreads - 1) / kThreads)), block(kThreads);
    if (vec) hipLaunchKernelGGL(x_to_yuv420p16_kernel<true>, grid, block, 0, stream, x, row_pixels, H, W, max_val(bit_depth), dist, yuv);
    else hipLaunchKernelGGL(x_to_yuv420p16_kernel<false>, grid, block, 0, stream, x, row_pixels, H, W, max_val(bit_depth), dist, yuv);
    hip_check(hipGetLastError(), "x_to_yuv420p16 launch");
}

}  // namespace dcvc
