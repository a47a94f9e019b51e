// wire_formats.hip - capture and file layouts ("wire formats": NV21, NV16 / P210, UYVY, YUY2 / Y210 / Y216, v210) <-> the carrier
// picture the rest of the library takes: wire_unpack in front of pix_to_x, wire_pack behind x_to_pix. A pass of
// its own that moves one picture's samples once; no arithmetic on a sample beyond the shift of a high-aligned u16.
//
// One picture, little-endian:
//   nv21   Y [H][W], then [H/2][W/2][2] as Cr, Cb; 8 bits                                 carrier NV12 (the pairs swapped)
//   nv16   Y [H][W], then [H][W/2][2] as Cb, Cr; above 8 bits u16, value in the high b bits (P210)       carrier YUV422P
//   uyvy   [H][W/2] x (Cb, Y0, Cr, Y1) bytes; 8 bits                                                    carrier YUV422P
//   yuy2   [H][W/2] x (Y0, Cb, Y1, Cr); above 8 bits u16, value in the high b bits (Y210 / Y212 / Y216)  carrier YUV422P
//   v210   rows of 128 ceil(W / 48) bytes; 6 pixels in four 32-bit words of three 10-bit fields at bits 0-9, 10-19, 20-29:
//          w0 = Cb0 Y0 Cr0, w1 = Y1 Cb2 Y2, w2 = Cr2 Y3 Cb4, w3 = Y4 Cr4 Y5; 10 bits                     carrier YUV422P
// The carrier is one picture in file layout as pix_to_x takes it: u8 at 8 bits, u16 above, LSB-aligned for YUV422P.
//   unpack: high-aligned samples are read as v >> (16 - b), v210 fields with & 1023; low bits, bits 30-31, fields past W and the
//           row padding are ignored. Samples above max_val are neither checked nor masked.
//   pack:   high-aligned samples are stored as (s << (16 - b)) & 0xFFFF, v210 fields as s & 1023; bits 30-31, the fields of a
//           last group past W and the row padding are written as zero: every byte of the wire picture is defined.
// Byte and u16 formats: one thread per 8 luma pixels of a row, 256-thread workgroups (picture_io.h). Both pictures are seen as
// two pieces of 8 samples per thread (the carrier's second piece: 4 Cb and 4 Cr, or 4 interleaved pairs); a compile-time table
// maps a carrier slot to its wire slot. v210: one thread per 4 groups (24 pixels: 64 bytes of wire, 48 + 24 + 24 bytes of u16
// planes), so that no two threads share a 32-bit word and a row's 128 ceil(W / 48) bytes are whole threads: on pack every byte
// of the row is written exactly once, padding included. VEC (host): W % 8 == 0 and both bases on the boundary of their largest
// access (8 samples; v210: 16 bytes) - one access per piece, element (v210 wire: byte) accesses elsewhere.
#include "picture_io.h"

namespace dcvc {

namespace {

constexpr int kThreads = kPictureThreads;

template <int BYTES> struct Raw;
template <> struct Raw<4> { typedef uint32_t type; };
template <> struct Raw<8> { typedef uint2 type; };
template <> struct Raw<16> { typedef uint4 type; };

// N samples of T behind an N sizeof(T)-aligned address in one access
template <typename T, int N>
__device__ __forceinline__ void load_n(const T* p, unsigned* v)
{
    typedef typename Raw<N * sizeof(T)>::type R;
    const R r = *reinterpret_cast<const R*>(p);
    const T* s = reinterpret_cast<const T*>(&r);
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = s[e];
}

template <typename T, int N>
__device__ __forceinline__ void store_n(T* p, const unsigned* v)
{
    typedef typename Raw<N * sizeof(T)>::type R;
    R r;
    T* s = reinterpret_cast<T*>(&r);
#pragma unroll
    for (int e = 0; e < N; ++e) s[e] = static_cast<T>(v[e]);
    *reinterpret_cast<R*>(p) = r;
}

// the first n of N samples, one by one; the others read as 0
template <typename T, int N>
__device__ __forceinline__ void load_elems(const T* p, int n, unsigned* v)
{
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = e < n ? p[e] : 0u;
}

template <typename T, int N>
__device__ __forceinline__ void store_elems(T* p, int n, const unsigned* v)
{
#pragma unroll
    for (int e = 0; e < N; ++e) {
        if (e < n) p[e] = static_cast<T>(v[e]);
    }
}

constexpr bool semi_planar(int wire) { return wire == kWireNv21 || wire == kWireNv16; }

// A thread's 8 luma pixels as 16 slots. Carrier: slots 0..7 the luma, then 4 Cb and 4 Cr (YUV422P) or 4 (Cb, Cr) pairs (NV12).
// Wire: slots 0..7 the luma and 8..15 the chroma pairs (semi-planar), or the 16 samples of the 4 packed pixel pairs.
// -> the wire slot that holds carrier slot j
constexpr int wire_slot(int wire, int j)
{
    if (j < 8) return semi_planar(wire) ? j : wire == kWireUyvy ? 2 * j + 1 : 2 * j;
    if (wire == kWireNv21) return 8 + ((j - 8) ^ 1);                      // NV12 pair (Cb, Cr) <-> (Cr, Cb)
    const int k = (j - 8) & 3, cr = (j - 8) >> 2;                         // YUV422P: Cb k (cr = 0) or Cr k
    if (wire == kWireNv16) return 8 + 2 * k + cr;
    return 4 * k + 2 * cr + (wire == kWireUyvy ? 0 : 1);
}

// one thread = 8 consecutive luma pixels of a row and the chroma samples that belong to them (NV21: written by the even row)
template <int WIRE, typename T, bool PACK, bool VEC>
__global__ void __launch_bounds__(kThreads) wire_kernel(const T* __restrict__ src, T* __restrict__ dst, int H, int W, int shift)
{
    constexpr bool SEMI = semi_planar(WIRE), NV = WIRE == kWireNv21;
    const unsigned wv = (W + 7) >> 3;
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;      // < 2^31 (wire_validate)
    if (i >= static_cast<unsigned>(H) * wv) return;
    const int h = static_cast<int>(i / wv), w0 = static_cast<int>(i - h * wv) * 8;
    const int n = VEC ? 8 : min(8, W - w0);                      // W is even: n is
    const size_t plane = static_cast<size_t>(H) * W, luma = static_cast<size_t>(h) * W + w0;
    const bool chroma_row = !NV || (h & 1) == 0;
    // the wire picture's two pieces of 8 samples and how many of each exist
    const size_t wa = SEMI ? luma : 2 * luma, wb = SEMI ? plane + static_cast<size_t>(NV ? h >> 1 : h) * W + w0 : wa + 8;
    const int wna = SEMI ? n : min(8, 2 * n), wnb = SEMI ? (chroma_row ? n : 0) : 2 * n - wna;
    // the carrier's: the luma, then 4 + 4 samples of two planes, or 8 interleaved ones
    const size_t cc = NV ? plane + static_cast<size_t>(h >> 1) * W + w0 : plane + static_cast<size_t>(h) * (W >> 1) + (w0 >> 1);
    const size_t cplane = static_cast<size_t>(H) * (W >> 1);
    unsigned c[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, v[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (PACK) {
        if constexpr (VEC) {
            load_n<T, 8>(src + luma, c);
            if constexpr (NV) {
                if (chroma_row) load_n<T, 8>(src + cc, c + 8);
            } else {
                load_n<T, 4>(src + cc, c + 8);
                load_n<T, 4>(src + cc + cplane, c + 12);
            }
        } else {
            load_elems<T, 8>(src + luma, n, c);
            if constexpr (NV) {
                load_elems<T, 8>(src + cc, chroma_row ? n : 0, c + 8);
            } else {
                load_elems<T, 4>(src + cc, n >> 1, c + 8);
                load_elems<T, 4>(src + cc + cplane, n >> 1, c + 12);
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) v[wire_slot(WIRE, j)] = c[j] << shift;      // the store keeps the low 8 or 16 bits
        if constexpr (VEC) {
            store_n<T, 8>(dst + wa, v);
            if (wnb) store_n<T, 8>(dst + wb, v + 8);
        } else {
            store_elems<T, 8>(dst + wa, wna, v);
            store_elems<T, 8>(dst + wb, wnb, v + 8);
        }
    } else {
        if constexpr (VEC) {
            load_n<T, 8>(src + wa, v);
            if (wnb) load_n<T, 8>(src + wb, v + 8);
        } else {
            load_elems<T, 8>(src + wa, wna, v);
            load_elems<T, 8>(src + wb, wnb, v + 8);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) c[j] = v[wire_slot(WIRE, j)] >> shift;
        if constexpr (VEC) {
            store_n<T, 8>(dst + luma, c);
            if constexpr (NV) {
                if (chroma_row) store_n<T, 8>(dst + cc, c + 8);
            } else {
                store_n<T, 4>(dst + cc, c + 8);
                store_n<T, 4>(dst + cc + cplane, c + 12);
            }
        } else {
            store_elems<T, 8>(dst + luma, n, c);
            if constexpr (NV) {
                store_elems<T, 8>(dst + cc, chroma_row ? n : 0, c + 8);
            } else {
                store_elems<T, 4>(dst + cc, n >> 1, c + 8);
                store_elems<T, 4>(dst + cc + cplane, n >> 1, c + 12);
            }
        }
    }
}

// ---------------------------------------------------------------- v210
constexpr int kV210Pixels = 24;      // per thread: 4 groups of 6 pixels, 16 words of wire

// rows of 128 ceil(W / 48) bytes = 2 ceil(W / 48) threads
inline long long v210_row_threads(int W) { return 2LL * ((W + 47) / 48); }

// The 12 fields of group g in wire order: Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5 over the group's 6 Y, 3 Cb, 3 Cr.
// A thread's samples are s[0..23] luma, s[24..35] Cb, s[36..47] Cr -> the slot of field f of group g
constexpr int v210_slot(int g, int f)
{
    constexpr int kind[12] = {1, 0, 2, 0, 1, 0, 2, 0, 1, 0, 2, 0};      // 0 Y, 1 Cb, 2 Cr
    constexpr int idx[12] = {0, 0, 0, 1, 1, 2, 1, 3, 2, 4, 2, 5};
    return kind[f] == 0 ? 6 * g + idx[f] : (kind[f] == 1 ? 24 : 36) + 3 * g + idx[f];
}

// one thread = 24 consecutive luma pixels of a row (of which n exist) and their 12 Cb and 12 Cr: 64 bytes of the wire row, which
// lie inside the row for every thread (the row is a multiple of 128 bytes). VEC: 16-byte accesses to the wire and, for a
// thread whose 24 pixels all exist, to the luma (8-byte to the chroma planes).
template <bool PACK, bool VEC>
__global__ void __launch_bounds__(kThreads) v210_kernel(const void* __restrict__ src, void* __restrict__ dst, int H, int W)
{
    const unsigned tr = static_cast<unsigned>(2 * ((W + 47) / 48));
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;      // < 2^31 (wire_validate)
    if (i >= static_cast<unsigned>(H) * tr) return;
    const int h = static_cast<int>(i / tr), t = static_cast<int>(i - h * tr);
    const int w0 = t * kV210Pixels, n = max(0, min(kV210Pixels, W - w0)), nc = n >> 1;      // W is even: n is
    const size_t plane = static_cast<size_t>(H) * W, cplane = static_cast<size_t>(H) * (W >> 1);
    const size_t luma = static_cast<size_t>(h) * W + w0, cb = plane + static_cast<size_t>(h) * (W >> 1) + (w0 >> 1), cr = cb + cplane;
    const size_t wire = (static_cast<size_t>(h) * tr + t) * 64;                             // bytes
    const bool whole = VEC && n == kV210Pixels;
    unsigned s[48], w[16];
    if constexpr (PACK) {
        const uint16_t* c = static_cast<const uint16_t*>(src);
        if (whole) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                load_n<uint16_t, 8>(c + luma + 8 * k, s + 8 * k);
                load_n<uint16_t, 4>(c + cb + 4 * k, s + 24 + 4 * k);
                load_n<uint16_t, 4>(c + cr + 4 * k, s + 36 + 4 * k);
            }
        } else {
            load_elems<uint16_t, 24>(c + luma, n, s);
            load_elems<uint16_t, 12>(c + cb, nc, s + 24);
            load_elems<uint16_t, 12>(c + cr, nc, s + 36);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                w[4 * g + k] = (s[v210_slot(g, 3 * k)] & 1023u) | (s[v210_slot(g, 3 * k + 1)] & 1023u) << 10 |
                               (s[v210_slot(g, 3 * k + 2)] & 1023u) << 20;
            }
        }
        uint8_t* o = static_cast<uint8_t*>(dst) + wire;
        if constexpr (VEC) {
#pragma unroll
            for (int k = 0; k < 4; ++k) reinterpret_cast<uint4*>(o)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
#pragma unroll
                for (int b = 0; b < 4; ++b) o[4 * k + b] = static_cast<uint8_t>(w[k] >> (8 * b));
            }
        }
    } else {
        if (n == 0) return;                                      // row padding
        const uint8_t* p = static_cast<const uint8_t*>(src) + wire;
        if constexpr (VEC) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint4 r = reinterpret_cast<const uint4*>(p)[k];
                w[4 * k] = r.x; w[4 * k + 1] = r.y; w[4 * k + 2] = r.z; w[4 * k + 3] = r.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                w[k] = static_cast<unsigned>(p[4 * k]) | static_cast<unsigned>(p[4 * k + 1]) << 8 |
                       static_cast<unsigned>(p[4 * k + 2]) << 16 | static_cast<unsigned>(p[4 * k + 3]) << 24;
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int f = 0; f < 12; ++f) s[v210_slot(g, f)] = (w[4 * g + f / 3] >> (10 * (f % 3))) & 1023u;
        }
        uint16_t* c = static_cast<uint16_t*>(dst);
        if (whole) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                store_n<uint16_t, 8>(c + luma + 8 * k, s + 8 * k);
                store_n<uint16_t, 4>(c + cb + 4 * k, s + 24 + 4 * k);
                store_n<uint16_t, 4>(c + cr + 4 * k, s + 36 + 4 * k);
            }
        } else {
            store_elems<uint16_t, 24>(c + luma, n, s);
            store_elems<uint16_t, 12>(c + cb, nc, s + 24);
            store_elems<uint16_t, 12>(c + cr, nc, s + 36);
        }
    }
}

// ---------------------------------------------------------------- host
bool known(int wire) { return wire >= kWireNv21 && wire <= kWireV210; }

// throws std::invalid_argument: an unknown format, a depth the format does not have, bad sides, a picture too large
void wire_validate(int wire, int bit_depth, int H, int W, const char* what)
{
    if (!known(wire)) throw std::invalid_argument(std::string(what) + ": unknown wire format " + std::to_string(wire));
    const bool any_depth = wire == kWireNv16 || wire == kWireYuy2;
    const int only = wire == kWireV210 ? 10 : 8;
    if (any_depth ? (bit_depth < 8 || bit_depth > 16) : bit_depth != only) {
        throw std::invalid_argument(std::string(what) + ": wire format " + std::to_string(wire) + " has " +
                                    (any_depth ? std::string("8..16") : std::to_string(only)) + " bits, got " + std::to_string(bit_depth));
    }
    picture_validate(H, W, what);
    // v210: one thread per 24 pixels of a padded row - more threads than one per 8 pixels below 16 columns
    if (wire == kWireV210 && static_cast<long long>(H) * v210_row_threads(W) + kThreads > (1LL << 31)) {
        throw std::invalid_argument(std::string(what) + ": picture too large");
    }
}

long long carrier_bytes(int bit_depth, int H, int W)
{
    const long long hc = H, wc = W / 2;                          // YUV422P and NV12 hold 2 H W samples and 1.5 H W
    return (static_cast<long long>(H) * W + 2 * hc * wc) * (bit_depth == 8 ? 1 : 2);
}

template <int WIRE, typename T, bool PACK>
void launch_wire(const void* src, void* dst, int H, int W, int shift, bool vec, hipStream_t stream)
{
    const dim3 grid(grid_of(H, W)), block(kThreads);
    const T* s = static_cast<const T*>(src);
    T* d = static_cast<T*>(dst);
    if (vec) hipLaunchKernelGGL((wire_kernel<WIRE, T, PACK, true>), grid, block, 0, stream, s, d, H, W, shift);
    else hipLaunchKernelGGL((wire_kernel<WIRE, T, PACK, false>), grid, block, 0, stream, s, d, H, W, shift);
}

template <bool PACK>
void convert(const void* src, int wire, int bit_depth, int H, int W, void* dst, const char* what, hipStream_t stream)
{
    wire_validate(wire, bit_depth, H, W, what);
    if (src == nullptr || dst == nullptr) throw std::invalid_argument(std::string(what) + ": null operand");
    const long long wbytes = wire_picture_bytes(wire, bit_depth, H, W);
    const long long cbytes = wire == kWireNv21 ? wbytes : carrier_bytes(bit_depth, H, W);
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
    const uintptr_t sn = static_cast<uintptr_t>(PACK ? cbytes : wbytes), dn = static_cast<uintptr_t>(PACK ? wbytes : cbytes);
    if (s0 < d0 + dn && d0 < s0 + sn) throw std::invalid_argument(std::string(what) + ": the source and the destination overlap");
    if (wire == kWireV210) {
        const bool vec = W % 8 == 0 && aligned(src, 16) && aligned(dst, 16);
        const long long threads = static_cast<long long>(H) * v210_row_threads(W);
        const dim3 grid(static_cast<unsigned>((threads + kThreads - 1) / kThreads)), block(kThreads);
        if (vec) hipLaunchKernelGGL((v210_kernel<PACK, true>), grid, block, 0, stream, src, dst, H, W);
        else hipLaunchKernelGGL((v210_kernel<PACK, false>), grid, block, 0, stream, src, dst, H, W);
    } else {
        const size_t piece = bit_depth == 8 ? 8 : 16;           // 8 samples
        const bool vec = W % 8 == 0 && aligned(src, piece) && aligned(dst, piece);
        const int shift = bit_depth > 8 ? 16 - bit_depth : 0;   // the u16 wire formats keep the value in the high bits
        switch (wire) {
        case kWireNv21: launch_wire<kWireNv21, uint8_t, PACK>(src, dst, H, W, shift, vec, stream); break;
        case kWireUyvy: launch_wire<kWireUyvy, uint8_t, PACK>(src, dst, H, W, shift, vec, stream); break;
        case kWireNv16:
            if (bit_depth == 8) launch_wire<kWireNv16, uint8_t, PACK>(src, dst, H, W, shift, vec, stream);
            else launch_wire<kWireNv16, uint16_t, PACK>(src, dst, H, W, shift, vec, stream);
            break;
        case kWireYuy2:
            if (bit_depth == 8) launch_wire<kWireYuy2, uint8_t, PACK>(src, dst, H, W, shift, vec, stream);
            else launch_wire<kWireYuy2, uint16_t, PACK>(src, dst, H, W, shift, vec, stream);
            break;
        }
    }
    hip_check(hipGetLastError(), (std::string(what) + " launch").c_str());
}

}  // namespace

int wire_carrier(int wire)
{
    if (!known(wire)) throw std::invalid_argument("wire_carrier: unknown wire format " + std::to_string(wire));
    return wire == kWireNv21 ? kPixNv12 : kPixYuv422p;
}

long long wire_picture_bytes(int wire, int bit_depth, int H, int W)
{
    wire_validate(wire, bit_depth, H, W, "wire_picture_bytes");
    if (wire == kWireV210) return static_cast<long long>(H) * 128 * ((W + 47) / 48);
    const long long samples = wire == kWireNv21 ? static_cast<long long>(H) * W * 3 / 2 : 2LL * H * W;
    return samples * (bit_depth == 8 ? 1 : 2);
}

void wire_unpack(const void* src, int wire, int bit_depth, int H, int W, void* carrier, hipStream_t stream)
{
    convert<false>(src, wire, bit_depth, H, W, carrier, "wire_unpack", stream);
}

void wire_pack(const void* carrier, int wire, int bit_depth, int H, int W, void* dst, hipStream_t stream)
{
    convert<true>(carrier, wire, bit_depth, H, W, dst, "wire_pack", stream);
}

}  // namespace dcvc
