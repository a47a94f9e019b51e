// crc32.hip - CRC-32 of up to 16 byte segments of one device buffer: the decoded-picture hash of
// dcvc --hash-log / --verify-hash, one segment per plane, all planes of a picture in the same launches.
//
// CRC-32/ISO-HDLC as zlib's crc32(): reflected polynomial 0xEDB88320, init 0xFFFFFFFF, final XOR 0xFFFFFFFF. A 32-bit word
// holds a polynomial over GF(2) with the coefficient of x^0 in bit 31 (zlib's convention: x^0 = 0x80000000). R(M), the raw CRC
// of a message M (init 0, no final XOR), is M(x) x^32 mod P. R is linear, R(A || B) = R(A) x^(8 |B|) + R(B), and blind to
// zero bytes in front of M; a register that holds s is s x^(8 n) after n zero bytes. So
//     crc32(M) = R(M) ^ 0xFFFFFFFF x^(8 |M|) ^ 0xFFFFFFFF                      (0 for the empty message)
//     R(M)     = XOR over chunks c of R(c) x^(8 bytes behind c),
// and XOR commutes: the result does not depend on the launch geometry or on the order the workgroups arrive in. Integer
// arithmetic only. Where each part is done:
//
//   init and final XOR  the host computes t = 0xFFFFFFFF x^(8 len) ^ 0xFFFFFFFF per segment (32 bits each, kernel arguments);
//                       a first launch of one 64-thread workgroup stores them into crc_out[0..n), which is also the zeroing.
//                       The init term is what makes the length count: without it two runs of zero bytes of different length
//                       would both hash to 0.
//   a thread's chunk    64 bytes, shift-xor steps in registers - crc ^= word, then 32 times crc = crc >> 1 ^ (P if bit 0) -
//                       no LDS tables: about 4 VALU operations a bit is 34 M lane-operations per megabyte, nothing to stage
//                       and nothing to conflict on. This arithmetic, not memory, bounds the call (12 us for a 1080p picture,
//                       33 us for 4K 16-bit, 8 ... 26 times the HBM floor and a hundredth of the copy to the host plus zlib's
//                       crc32 it replaces: DESIGN.md 19). A segment is laid on a grid of 16-byte
//                       words of its ADDRESS: pad = address & 15 virtual zero bytes stand in front of it (leading zeros do not
//                       change R), so every word that lies inside the segment is one aligned 16-byte load; the words that hold
//                       the segment's first and last bytes are read byte by byte, only the bytes inside the segment. Bytes
//                       past the segment's end, up to the end of the chunk, are fed as zeros: every chunk then ends on its
//                       64-byte boundary and every workgroup on its 16 KiB boundary, and z, the number of such zero bytes of
//                       the segment, is divided out again below.
//   inside a workgroup  256 threads = 16 KiB. Thread t multiplies its R by x^(8 * 64 * (255 - t)) - a 256-entry table in
//                       constant memory, one carry-less multiply mod P in software (32 shift-xor steps) - then a plain XOR
//                       down the wave (64 lanes, __shfl_xor) and across the 4 waves through 16 bytes of LDS.
//   across workgroups   workgroup w of a segment has 8 e bits behind it, e = pad + len - 16384 (w + 1). Wave 0 builds x^(8 e):
//                       lane k holds x^(2^(k + 3)) (a 32-entry table, x^(2^32) = x mod P) if bit k of e is set, else x^0, and
//                       the 64 lanes are multiplied together in 6 butterfly levels. The last workgroup (e = -z) takes x^(-8 z)
//                       from the host instead, = x^(2^32 - 1 - 8 z mod (2^32 - 1)): P is irreducible, the order of x divides
//                       2^32 - 1 (the host checks the product with x^(8 z) to be x^0). One atomic XOR per workgroup onto
//                       crc_out[segment].
//
// Two launches per call, or one when every segment is empty; no allocation, no host synchronisation. Offsets, lengths and
// the pointer are validated before the first launch (crc32_validate). crc32_combine is host code on the same arithmetic.
#include "ops.h"

namespace dcvc {

namespace {

constexpr uint32_t kPoly = 0xEDB88320u;
constexpr uint32_t kOne = 0x80000000u;         // x^0
constexpr int kThreads = 256;
constexpr int kChunk = 64;                     // bytes of one thread
constexpr long long kGroupBytes = static_cast<long long>(kThreads) * kChunk;

// a(x) b(x) mod P
__host__ __device__ constexpr uint32_t mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        p ^= b & (0u - ((a >> (31 - i)) & 1u));
        b = (b >> 1) ^ (kPoly & (0u - (b & 1u)));
    }
    return p;
}

struct Tables {
    uint32_t x2n[32];            // x^(2^k) mod P
    uint32_t lane[kThreads];     // x^(8 * kChunk * (kThreads - 1 - t)) mod P
};

constexpr Tables make_tables()
{
    Tables t{};
    uint32_t p = kOne >> 1;      // x^1
    for (int k = 0; k < 32; ++k) {
        t.x2n[k] = p;
        p = mulmod(p, p);
    }
    uint32_t step = t.x2n[9];    // x^(8 * 64) = x^512
    static_assert(8 * kChunk == 512, "the lane table's step is x^(2^9)");
    uint32_t q = kOne;
    for (int i = kThreads - 1; i >= 0; --i) {
        t.lane[i] = q;
        q = mulmod(q, step);
    }
    return t;
}

constexpr Tables kHostTables = make_tables();
__device__ const Tables kTables = make_tables();

// x^(8 n) mod P, n >= 0
uint32_t xpow8(unsigned long long n)
{
    uint32_t p = kOne;
    for (int k = 3; n != 0; n >>= 1, ++k) {
        if (n & 1ull) p = mulmod(kHostTables.x2n[k & 31], p);
    }
    return p;
}

// x^(-8 z) mod P
uint32_t xpow8_inverse(unsigned long long z)
{
    const unsigned long long ord = 0xFFFFFFFFull;                  // x^(2^32 - 1) = x^0
    const unsigned long long e = (ord - (z % ord) * 8 % ord) % ord;
    uint32_t p = kOne;
    unsigned long long n = e;
    for (int k = 0; n != 0; n >>= 1, ++k) {
        if (n & 1ull) p = mulmod(kHostTables.x2n[k & 31], p);
    }
    if (mulmod(p, xpow8(z)) != kOne) throw std::logic_error("crc32: x^(-8 z) is no inverse");
    return p;
}

struct Segment {
    const uint8_t* grid;         // the segment's address rounded down to 16 bytes: virtual byte v of the segment is grid[v]
    long long end;               // pad + len: the virtual bytes [pad, end) are the segment
    unsigned first_group;        // the segment's first workgroup in the launch
    unsigned pad;
    uint32_t inverse;            // x^(-8 z), z = groups * 16384 - end
};

struct Params {
    Segment seg[kCrc32MaxSegments];
    uint32_t init[kCrc32MaxSegments];
    int n;
};

template <int BITS>
__device__ __forceinline__ uint32_t steps(uint32_t crc)
{
#pragma unroll
    for (int i = 0; i < BITS; ++i) crc = (crc >> 1) ^ (kPoly & (0u - (crc & 1u)));
    return crc;
}

__global__ void crc32_init_kernel(Params p, uint32_t* __restrict__ out)
{
    if (static_cast<int>(threadIdx.x) < p.n) out[threadIdx.x] = p.init[threadIdx.x];
}

__global__ void __launch_bounds__(kThreads) crc32_kernel(Params p, uint32_t* __restrict__ out)
{
    __shared__ uint32_t scratch[kThreads / 64];
    // the segment of this workgroup: the last one that starts at or before it (empty segments own no workgroup)
    int s = 0;
    for (int k = 1; k < p.n; ++k) {
        if (p.seg[k].first_group <= blockIdx.x) s = k;
    }
    const uint8_t* grid = p.seg[s].grid;
    const long long end = p.seg[s].end;
    const long long pad = p.seg[s].pad;
    const long long w = static_cast<long long>(blockIdx.x - p.seg[s].first_group);
    const long long c0 = w * kGroupBytes + static_cast<long long>(threadIdx.x) * kChunk;
    uint32_t crc = 0;
    if (c0 < end) {
        if (c0 >= pad && c0 + kChunk <= end) {
            const uint4* src = reinterpret_cast<const uint4*>(grid + c0);
            const uint4 q0 = src[0], q1 = src[1], q2 = src[2], q3 = src[3];
            const uint32_t word[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
#pragma unroll
            for (int i = 0; i < 16; ++i) crc = steps<32>(crc ^ word[i]);
        } else {
            // the chunk holds the segment's first or last byte
            for (int i = 0; i < kChunk / 16; ++i) {
                const long long v = c0 + 16 * i;
                if (v >= pad && v + 16 <= end) {
                    const uint4 q = *reinterpret_cast<const uint4*>(grid + v);
                    crc = steps<32>(crc ^ q.x);
                    crc = steps<32>(crc ^ q.y);
                    crc = steps<32>(crc ^ q.z);
                    crc = steps<32>(crc ^ q.w);
                } else {
                    for (long long b = v; b < v + 16; ++b) {
                        if (b < pad) continue;                                   // in front of the segment: crc is still 0
                        crc = steps<8>(b < end ? crc ^ grid[b] : crc);           // behind it: a zero byte
                    }
                }
            }
        }
        crc = mulmod(crc, kTables.lane[threadIdx.x]);
    }
    for (int o = 32; o > 0; o >>= 1) crc ^= __shfl_xor(crc, o);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = crc;
    __syncthreads();
    if (threadIdx.x < 64) {
        // x^(8 e), e = the bytes behind this workgroup; the segment's last workgroup: x^(-8 z)
        const long long e = end - (w + 1) * kGroupBytes;
        uint32_t m = kOne;
        if (e > 0) {
            if ((static_cast<unsigned long long>(e) >> threadIdx.x) & 1ull) m = kTables.x2n[(threadIdx.x + 3) & 31];
            for (int o = 32; o > 0; o >>= 1) m = mulmod(m, __shfl_xor(m, o));
        } else {
            m = p.seg[s].inverse;
        }
        if (threadIdx.x == 0) {
            uint32_t t = 0;
            for (int k = 0; k < kThreads / 64; ++k) t ^= scratch[k];
            t = mulmod(t, m);
            if (t) atomicXor(out + s, t);
        }
    }
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

constexpr long long kMaxBytes = 1ll << 44;     // offset + length of a segment; 16 segments stay below 2^31 workgroups

}  // namespace

void crc32_validate(const Crc32Desc& d)
{
    if (d.base == nullptr || d.offsets == nullptr || d.lengths == nullptr || d.out == nullptr) {
        throw std::invalid_argument("crc32: null operand");
    }
    if (d.n < 1 || d.n > kCrc32MaxSegments) {
        throw std::invalid_argument("crc32: n must be in 1.." + std::to_string(kCrc32MaxSegments) + ", got " + std::to_string(d.n));
    }
    if (!aligned(d.out, 4)) throw std::invalid_argument("crc32: crc_out must be 4-byte aligned");
    for (int k = 0; k < d.n; ++k) {
        if (d.offsets[k] < 0 || d.lengths[k] < 0) {
            throw std::invalid_argument("crc32: segment " + std::to_string(k) + " has a negative offset or length (" +
                                        std::to_string(d.offsets[k]) + ", " + std::to_string(d.lengths[k]) + ")");
        }
        if (d.offsets[k] > kMaxBytes || d.lengths[k] > kMaxBytes - d.offsets[k]) {
            throw std::invalid_argument("crc32: segment " + std::to_string(k) + " ends above 2^44 bytes");
        }
    }
}

void crc32_segments(const Crc32Desc& d, hipStream_t stream)
{
    crc32_validate(d);
    Params p{};
    p.n = d.n;
    unsigned long long groups = 0;
    for (int k = 0; k < d.n; ++k) {
        const uint8_t* at = static_cast<const uint8_t*>(d.base) + d.offsets[k];
        const unsigned pad = static_cast<unsigned>(reinterpret_cast<uintptr_t>(at) & 15);
        const long long end = static_cast<long long>(pad) + d.lengths[k];
        const unsigned long long own = d.lengths[k] == 0 ? 0 : static_cast<unsigned long long>((end + kGroupBytes - 1) / kGroupBytes);
        Segment& s = p.seg[k];
        s.grid = at - pad;
        s.end = end;
        s.pad = pad;
        s.first_group = static_cast<unsigned>(groups);
        s.inverse = own ? xpow8_inverse(own * static_cast<unsigned long long>(kGroupBytes) - static_cast<unsigned long long>(end)) : kOne;
        p.init[k] = mulmod(0xFFFFFFFFu, xpow8(static_cast<unsigned long long>(d.lengths[k]))) ^ 0xFFFFFFFFu;
        groups += own;       // <= 16 * (2^44 / 2^14 + 1) < 2^31
    }
    uint32_t* out = static_cast<uint32_t*>(d.out);
    hipLaunchKernelGGL(crc32_init_kernel, dim3(1), dim3(64), 0, stream, p, out);
    hip_check(hipGetLastError(), "crc32 init launch");
    if (groups == 0) return;
    hipLaunchKernelGGL(crc32_kernel, dim3(static_cast<unsigned>(groups)), dim3(kThreads), 0, stream, p, out);
    hip_check(hipGetLastError(), "crc32 launch");
}

uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, long long len_b)
{
    if (len_b < 0) throw std::invalid_argument("crc32_combine: negative length");
    if (len_b == 0) return crc_a;                  // B is empty
    return mulmod(crc_a, xpow8(static_cast<unsigned long long>(len_b))) ^ crc_b;
}

}  // namespace dcvc
