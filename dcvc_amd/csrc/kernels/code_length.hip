// code_length.hip - the size of a stream from the symbols where they lie: a gather from the cost tables of
// rans/code_length.h and an integer sum per picture. After the encoder's symbol kernels the stream's length is decided;
// this makes it known without the symbol copy and the host coder.
//
// Integer sums only (64-bit partials per thread, wave reduction, one atomic add per workgroup): the result does not depend
// on the order of the additions, so it is the same number on every run and for every grid. The cost tables (128 KB for the
// y family, 64 KB for the z rows of one q_index) are read through the cache; no LDS staging.
#include "ops.h"

namespace dcvc {

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 8;
constexpr int kBlockElems = kThreads * kPerThread;
constexpr int kMaxBlocks = 1024;        // per picture; larger pictures walk in grid strides

typedef short short8 __attribute__((ext_vector_type(8)));

// the block's sum in thread 0
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* lds)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return lds[0] + lds[1] + lds[2] + lds[3];
}

__global__ void __launch_bounds__(kThreads)
code_length_y_kernel(const CodeLengthY d)
{
    __shared__ unsigned long long lds[4];
    const int16_t* sym = d.sym + blockIdx.y * d.sym_stride;
    const uint8_t* cond = d.cond ? d.cond + blockIdx.y * d.cond_stride : nullptr;
    int count = d.count;
    if (d.totals) {
        const int32_t* t = d.totals + static_cast<size_t>(blockIdx.y) * d.totals_stride;
        int s = 0;
        for (int k = 0; k < d.n_totals; ++k) s += t[k];
        count = s < 0 ? 0 : (s < d.count ? s : d.count);      // never beyond what the caller sized the buffer for
    }
    unsigned long long cost = 0, kept = 0;
    for (long long e0 = (static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x) * kPerThread; e0 < count;
         e0 += static_cast<long long>(gridDim.x) * kBlockElems) {
        const unsigned flags = cond ? cond[e0 >> 3] : 0xFFu;
        short s8[kPerThread];
        if (e0 + kPerThread <= count) {
            const short8 v = *reinterpret_cast<const short8*>(sym + e0);
#pragma unroll
            for (int i = 0; i < kPerThread; ++i) s8[i] = v[i];
        } else {
#pragma unroll
            for (int i = 0; i < kPerThread; ++i) s8[i] = e0 + i < count ? sym[e0 + i] : static_cast<short>(0);
        }
#pragma unroll
        for (int i = 0; i < kPerThread; ++i) {
            const unsigned c = static_cast<unsigned short>(s8[i]);
            const unsigned idx = c & 0xFFu, col = c >> 8;               // (q << 8) + idx: q's low byte is the column
            const bool on = e0 + i < count && ((flags >> i) & 1u) != 0 && idx < static_cast<unsigned>(d.num_cdf);
            if (on) {
                cost += d.table[idx * 256u + col];
                ++kept;
            }
        }
    }
    const unsigned long long c = block_sum_u64(cost, lds);
    __syncthreads();
    const unsigned long long k = block_sum_u64(kept, lds);
    if (threadIdx.x == 0) {
        unsigned long long* out = d.out + static_cast<size_t>(blockIdx.y) * d.out_stride;
        if (c) atomicAdd(out, c);
        if (k && d.kept_slot >= 0) atomicAdd(out + d.kept_slot, k);
    }
}

__global__ void __launch_bounds__(kThreads)
code_length_z_kernel(const CodeLengthZ d)
{
    __shared__ unsigned long long lds[4];
    const int8_t* z = d.z + static_cast<size_t>(blockIdx.y) * d.count;
    unsigned long long cost = 0;
    for (long long i = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; i < d.count;
         i += static_cast<long long>(gridDim.x) * kThreads) {
        const unsigned row = static_cast<unsigned>(i % d.ch);
        const unsigned col = static_cast<unsigned>(z[i] + 64) & 127u;
        cost += d.table[row * 128u + col];
    }
    const unsigned long long c = block_sum_u64(cost, lds);
    if (threadIdx.x == 0 && c) atomicAdd(d.out + static_cast<size_t>(blockIdx.y) * d.out_stride, c);
}

}  // namespace

void code_length_y(const CodeLengthY& d, hipStream_t stream)
{
    if (d.n < 1 || d.n > 65535) throw std::invalid_argument("code_length_y: batch size out of range");
    if (d.count < 0 || d.num_cdf < 1 || d.num_cdf > 256) throw std::invalid_argument("code_length_y: bad count or table");
    if (d.sym == nullptr || d.table == nullptr || d.out == nullptr) throw std::invalid_argument("code_length_y: null pointer");
    if (reinterpret_cast<uintptr_t>(d.sym) % 16 != 0 || d.sym_stride % 8 != 0) {
        throw std::invalid_argument("code_length_y: symbols must be 16-byte aligned, picture stride a multiple of 8");
    }
    if (d.totals != nullptr && (d.n_totals < 1 || d.n_totals > 4)) throw std::invalid_argument("code_length_y: 1..4 totals");
    if (d.kept_slot >= d.out_stride || d.out_stride < 1) throw std::invalid_argument("code_length_y: bad output layout");
    if (d.count == 0) return;
    const int blocks = (d.count + kBlockElems - 1) / kBlockElems;
    hipLaunchKernelGGL(code_length_y_kernel, dim3(blocks < kMaxBlocks ? blocks : kMaxBlocks, d.n), dim3(kThreads), 0, stream, d);
    hip_check(hipGetLastError(), "code_length_y launch");
}

void code_length_z(const CodeLengthZ& d, hipStream_t stream)
{
    if (d.n < 1 || d.n > 65535) throw std::invalid_argument("code_length_z: batch size out of range");
    if (d.count < 0 || d.ch < 1) throw std::invalid_argument("code_length_z: bad count or channel count");
    if (d.z == nullptr || d.table == nullptr || d.out == nullptr || d.out_stride < 1) throw std::invalid_argument("code_length_z: null pointer");
    if (d.count == 0) return;
    const int blocks = (d.count + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(code_length_z_kernel, dim3(blocks < kMaxBlocks ? blocks : kMaxBlocks, d.n), dim3(kThreads), 0, stream, d);
    hip_check(hipGetLastError(), "code_length_z launch");
}

}  // namespace dcvc
