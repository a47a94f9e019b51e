// Host side of the two block kernels (dcb_nsplit8_kernel.h, dcb_pair8_kernel.h): weight packing, and the N-split kernel's shape
// dispatch. (Includes no kernel: the instantiations live in units of their own.)
#include "dcb_shapes.h"
#include "dcb_wave_share.h"

#include <vector>

namespace dcvc {

using namespace nsplit;
using namespace nsplit8;

namespace {

// ------------------------------------------------------------------------------------ weight packing
// [waves][fragments][64 lanes][8 halves]: fragment = the MFMA "A" operand of one (32-channel tile, 16-deep k-slice):
// lane l holds row (l & 31), k = 8 (l >> 5) .. + 7. Order inside a wave's stream = the order the kernel consumes.
// the kernel's streams (dcb_nsplit8_kernel.h): waves 0 .. 3, then 4 .. 7; which tiles of a layer a wave owns is dcb_wave_share.h's;
// a layer's fragments in a wave's stream: k-slice major, the wave's tiles inside; ffn.0: its tiles in passes of 2

// unit u (16 bytes) of a stream whose waves 0 .. 3 hold f_hi fragments each and 4 .. 7 f_lo
struct StreamPos { int wave, f, lane; };
__device__ StreamPos stream_pos(long long u, int f_hi, int f_lo)
{
    const int F = static_cast<int>(u >> 6);
    const bool hiw = F < 4 * f_hi;
    return {hiw ? F / f_hi : 4 + (F - 4 * f_hi) / f_lo, hiw ? F % f_hi : (F - 4 * f_hi) % f_lo, static_cast<int>(u & 63)};
}

__device__ half8 load_fragment(const half_t* w, int K, int tile, int ks, int lane)
{
    return *reinterpret_cast<const half8*>(w + static_cast<size_t>(32 * tile + (lane & 31)) * K + 16 * ks + 8 * (lane >> 5));
}

// fragment f of wave `wave`'s share of the layer w [N][K]; a wave without a share walks tiles of zeros (block width 192: waves 6, 7)
__device__ half8 layer_fragment(const half_t* w, int K, const WaveShare& s, int wave, int f, int lane)
{
    const int nt = s.tiles_of(wave >= 4);
    if (!s.on(wave)) return half8{0, 0, 0, 0, 0, 0, 0, 0};
    return load_fragment(w, K, s.first_tile(wave) + f % nt, f / nt, lane);
}

// one layer [N][K] as a stream of its own: dc.0, a closing conv, the adaptor
__global__ void pack_layer_kernel(const half_t* w, int K, WaveShare s, half8* out)
{
    const int KS = K / 16;
    const long long u = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (u >= 64LL * s.slots() * KS) return;
    const StreamPos at = stream_pos(u, s.hi * KS, s.lo * KS);
    out[u] = layer_fragment(w, K, s, at.wave, at.f, at.lane);
}

// dc.3 [C][CI] | ffn.0 [4 CI][C] | ffn.2 [C][CI] per wave
__global__ void pack_main8_kernel(const half_t* w3, const half_t* w0, const half_t* w2, int C, int CI, half8* out)
{
    const int KS_C = C / 16, KS_I = CI / 16, TP = 2;
    const WaveShare sc = WaveShare::block_layer(C);
    const Ffn0Share s0(CI);
    const int FM_HI = 2 * sc.hi * KS_I + 2 * s0.hi * KS_C, FM_LO = 2 * sc.lo * KS_I + 2 * s0.lo * KS_C;
    const long long u = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (u >= 4LL * (FM_HI + FM_LO) * 64) return;
    const StreamPos at = stream_pos(u, FM_HI, FM_LO);
    const bool upper = at.wave >= 4;
    const int F_DC3 = sc.tiles_of(upper) * KS_I, F_FFN0 = 2 * s0.pairs_of(upper) * KS_C;
    if (at.f < F_DC3) {
        out[u] = layer_fragment(w3, CI, sc, at.wave, at.f, at.lane);
    } else if (at.f < F_DC3 + F_FFN0) {
        const int g = at.f - F_DC3, pass = g / (TP * KS_C), r = g % (TP * KS_C);
        out[u] = load_fragment(w0, C, s0.first_tile(at.wave) + TP * pass + r % TP, r / TP, at.lane);
    } else {
        out[u] = layer_fragment(w2, CI, sc, at.wave, at.f - F_DC3 - F_FFN0, at.lane);
    }
}

size_t layer_halves(const WaveShare& s, int k) { return 1ull * s.slots() * (k / 16) * 512; }

void pack_layer(const half_t* w, int k, const WaveShare& s, half_t* out, hipStream_t stream)
{
    const long long units = static_cast<long long>(layer_halves(s, k) / 8);
    hipLaunchKernelGGL(pack_layer_kernel, dim3(static_cast<unsigned>((units + 255) / 256)), dim3(256), 0, stream, w, k, s, reinterpret_cast<half8*>(out));
    hip_check(hipGetLastError(), "dcb_nsplit pack");
}

long long* g_ns_timeline = nullptr;
// tuning aid (tools/probes/core_bench.hip -w): launches of a shape that has the variant run it with the depthwise conv inside, on these operands
const half_t* g_dw_hook_t1 = nullptr;
const half_t* g_dw_hook_taps = nullptr;
int g_dw_hook_width = 0;

}  // namespace

bool dcb_nsplit_shape(int c, int ci) { return find_block(c, ci) != nullptr; }

void dcb_nsplit_check_shape(int c, int ci)
{
    static const std::string text = [] {
        std::string t = "dcb_nsplit: (block width, inner width) must be ";
        for (int i = 0; i < N_BLOCK_SHAPES; ++i) {
            t += std::string(i == 0 ? "(" : i == N_BLOCK_SHAPES - 1 ? " or (" : ", (") + std::to_string(BLOCK_SHAPES[i].c) + ", " +
                 std::to_string(BLOCK_SHAPES[i].ci) + ")";
        }
        return t;
    }();
    if (!dcb_nsplit_shape(c, ci)) throw std::invalid_argument(text);
}

// widths of a chain-closing conv the kernel of a block shape is instantiated for
bool dcb_nsplit_fin_supported(int c, int ci, int nn)
{
    static const bool off = [] { const char* e = getenv("DCVC_NSPLIT_FIN"); return e != nullptr && atoi(e) == 0; }();   // A/B: the closing convs as launches of their own
    const BlockShape* s = find_block(c, ci);
    return !off && s != nullptr && has_fin(*s, nn);
}

static bool nsplit_wide(int pixels, const BlockShape& s)
{
    // DCVC_NSPLIT_PX=32: 32-pixel workgroups everywhere (A/B: twice the tiles per workgroup, half the work per weight byte)
    static const bool narrow_all = [] { const char* e = getenv("DCVC_NSPLIT_PX"); return e != nullptr && atoi(e) == 32; }();
    return pixels >= DCB_WIDE_PIXELS && s.px64 && !narrow_all;
}

// block shapes the kernel is also instantiated for with the block's depthwise conv inside
bool dcb_nsplit_dw_supported(int c, int ci, int pixels)
{
    static const bool off = [] { const char* e = getenv("DCVC_NSPLIT_DW"); return e != nullptr && atoi(e) == 0; }();   // A/B: the depthwise conv as a launch of its own
    const BlockShape* s = find_block(c, ci);
    if (off || pixels <= 0 || s == nullptr) return false;
    return s->dw == DwInside::any_px || (s->dw == DwInside::px32 && !nsplit_wide(pixels, *s));
}

void dcb_nsplit_dw_hook(const half_t* t1, const half_t* wdw, int width)
{
    g_dw_hook_t1 = t1; g_dw_hook_taps = wdw; g_dw_hook_width = width;
}

void dcb_nsplit_timeline_buffer(long long* device_buffer)
{
    g_ns_timeline = device_buffer;
}

// stream sizes in halves (a fragment = 512): the waves' slots of every layer, the zero tiles of waves without a share included
size_t dcb_nsplit_main_halves(int c, int ci)
{
    const Ffn0Share s0(ci);
    return 2 * layer_halves(WaveShare::block_layer(c), ci) + 2ull * 4 * (s0.hi + s0.lo) * (c / 16) * 512;
}
size_t dcb_nsplit_dc0_halves(int c, int ci) { return layer_halves(WaveShare::block_layer(ci), c); }
size_t dcb_nsplit_fin_halves(int c, int nn) { return layer_halves(WaveShare::by_wave(nn), c); }
size_t dcb_pair_adaptor_halves(int cin, int c) { return layer_halves(WaveShare::block_layer(c), cin); }

bool dcb_nsplit_fin_packable(int c, int nn) { return c % 128 == 0 && nn % 32 == 0 && nn >= 128; }

void dcb_nsplit_pack_fin(const half_t* w, int c, int nn, half_t* out, hipStream_t stream)
{
    if (!dcb_nsplit_fin_packable(c, nn)) throw std::invalid_argument("dcb_nsplit: unsupported closing conv");
    pack_layer(w, c, WaveShare::by_wave(nn), out, stream);
}

void dcb_nsplit_pack_main(const half_t* w3, const half_t* w0, const half_t* w2, int c, int ci, half_t* out, hipStream_t stream)
{
    if (!dcb_nsplit_shape(c, ci)) throw std::invalid_argument("dcb_nsplit: unsupported block shape");
    const long long units = static_cast<long long>(dcb_nsplit_main_halves(c, ci) / 8);
    hipLaunchKernelGGL(pack_main8_kernel, dim3(static_cast<unsigned>((units + 255) / 256)), dim3(256), 0,
                       stream, w3, w0, w2, c, ci, reinterpret_cast<half8*>(out));
    hip_check(hipGetLastError(), "dcb_nsplit pack");
}

void dcb_nsplit_pack_dc0(const half_t* w1, int c, int ci, half_t* out, hipStream_t stream)
{
    if (!dcb_nsplit_shape(c, ci)) throw std::invalid_argument("dcb_nsplit: unsupported block shape");
    pack_layer(w1, c, WaveShare::block_layer(ci), out, stream);
}

// [C][CIN], shared as the block's C-wide layers (dcb_pair8_kernel.h)
void dcb_pair_pack_adaptor(const half_t* wa, int cin, int c, half_t* out, hipStream_t stream)
{
    if (c % 64 != 0 || cin % 64 != 0) throw std::invalid_argument("dcb_pair: unsupported adaptor shape");
    pack_layer(wa, cin, WaveShare::block_layer(c), out, stream);
}

int dcb_nsplit_mode()
{
    // DCVC_NSPLIT: 0 = never (A/B against dcb_core / dcb_tail / the launch sequence), 1 = full-width blocks only,
    // unset / 2 = wherever the shape allows (the half-width `dcb2` blocks of the inter models too)
    static const int mode = [] { const char* e = getenv("DCVC_NSPLIT"); return e != nullptr ? atoi(e) : 2; }();
    return mode;
}

bool dcb_nsplit_supported(int c, int cdc, int cffn)
{
    static const bool core_off = [] { const char* e = getenv("DCVC_NO_DCB_CORE"); return e != nullptr && atoi(e) != 0; }();
    if (core_off || dcb_nsplit_mode() == 0 || cdc != cffn || !dcb_nsplit_shape(c, cdc)) return false;
    return cdc == c || dcb_nsplit_mode() >= 2;
}

// ------------------------------------------------------------------------------------ dispatch: every launch8 the rows of BLOCK_SHAPES
// allow, by (shape, workgroup size, NEXT slot, depthwise inside). Each is named here, so each must exist in some
// dcb_nsplit8_<shape>*.hip (dcb_shapes.h)
namespace {

using Launch8 = void (*)(const NsParams&, hipStream_t);
struct Variant { int c, ci, pxt, next, dw; Launch8 launch; };

// NEXT = 0 (nothing behind ffn.2), 1 (dc.0 of the next block), then the row's closing convs
template <int I, int PXT, int DW, int J = -2>
void add_nexts(std::vector<Variant>& v)
{
    constexpr BlockShape S = BLOCK_SHAPES[I];
    constexpr int NEXT = J < 0 ? J + 2 : S.fins[J];
    if constexpr (J < 0 || NEXT != 0) v.push_back({S.c, S.ci, PXT, NEXT, DW, &nsplit8::launch8<S.c, S.ci, PXT, NEXT, DW>});
    if constexpr (J < 2) add_nexts<I, PXT, DW, J + 1>(v);
}

template <int I = 0>
void add_rows(std::vector<Variant>& v)
{
    if constexpr (I < N_BLOCK_SHAPES) {
        constexpr BlockShape S = BLOCK_SHAPES[I];
        add_nexts<I, 1, 0>(v);
        if constexpr (S.px64) add_nexts<I, 2, 0>(v);
        if constexpr (S.dw != DwInside::none) add_nexts<I, 1, 1>(v);
        if constexpr (S.dw == DwInside::any_px && S.px64) add_nexts<I, 2, 1>(v);
        add_rows<I + 1>(v);
    }
}

}  // namespace

void dcb_nsplit(const DcbNsplitDesc& desc, hipStream_t stream)
{
    DcbNsplitDesc d = desc;
    if (g_dw_hook_t1 != nullptr && d.t1 == nullptr && dcb_nsplit_dw_supported(d.c, d.ci, d.pixels) && d.pixels % g_dw_hook_width == 0) {
        d.t2 = nullptr; d.t1 = g_dw_hook_t1; d.wdw = g_dw_hook_taps; d.width = g_dw_hook_width;
    }
    dcb_nsplit_check_shape(d.c, d.ci);
    if (d.pixels <= 0) throw std::invalid_argument("dcb_nsplit: empty problem");
    if ((d.ldt % 8) || (d.ldx % 8) || (d.ldy % 8) || (d.wnext && d.ldt1 % 8)) {
        throw std::invalid_argument("dcb_nsplit: leading dimensions must be multiples of 8 channels");
    }
    if (d.t1 != nullptr) {
        if (d.t2 != nullptr) throw std::invalid_argument("dcb_nsplit: either the depthwise conv's output (t2) or its input (t1)");
        if (!dcb_nsplit_dw_supported(d.c, d.ci, d.pixels)) throw std::invalid_argument("dcb_nsplit: no kernel with the depthwise conv inside for this block shape and size");
        if (!d.wdw || d.width <= 0 || d.pixels % d.width != 0) throw std::invalid_argument("dcb_nsplit: depthwise conv inside needs its taps and the picture's width");
        if (d.t1 == d.t1n) throw std::invalid_argument("dcb_nsplit: dc.0's output for the next block must not overwrite this block's (neighbouring workgroups read it)");
    }
    if ((!d.t2 && !d.t1) || !d.x || !d.wmain || !d.b3 || !d.b0 || !d.b2 || (!d.y && !d.wfin) || (d.wnext && (!d.b1n || !d.t1n))) {
        throw std::invalid_argument("dcb_nsplit: missing operand");
    }
    if (d.wfin != nullptr) {
        if (d.wnext != nullptr) throw std::invalid_argument("dcb_nsplit: a block either hands dc.0 to the next block or closes the chain");
        if (!dcb_nsplit_fin_supported(d.c, d.ci, d.nfin)) throw std::invalid_argument("dcb_nsplit: no kernel for this closing conv");
        if (!d.bfin || !d.yfin || d.ldyfin % 8) throw std::invalid_argument("dcb_nsplit: closing conv needs bias, output and a leading dimension in units of 8");
    }
    NsParams p{};
    p.t2 = d.t2; p.ldt = d.ldt; p.x = d.x; p.ldx = d.ldx;
    p.t1 = d.t1; p.wdw = d.wdw; p.W = d.width;
    p.wmain = reinterpret_cast<const half8*>(d.wmain); p.wnext = reinterpret_cast<const half8*>(d.wnext);
    p.b3 = d.b3; p.b0 = d.b0; p.b2 = d.b2; p.b1n = d.b1n; p.q = d.q; p.q2 = d.q2;
    p.wsilu = wsilu_table_device();
    p.y = d.y; p.ldy = d.ldy; p.t1n = d.t1n; p.ldt1 = d.ldt1; p.M = d.pixels; p.shortcut = d.shortcut ? 1 : 0;
    p.timeline = g_ns_timeline;
    if (d.wfin != nullptr) {      // the NEXT slot holds the chain's closing conv
        p.wnext = reinterpret_cast<const half8*>(d.wfin); p.b1n = d.bfin; p.qf = d.qfin; p.t1n = d.yfin; p.ldt1 = d.ldyfin;
    }
    const bool wide = nsplit_wide(d.pixels, *find_block(d.c, d.ci));
    const int next = d.wfin != nullptr ? d.nfin : d.wnext != nullptr ? 1 : 0;
    static const std::vector<Variant> variants = [] { std::vector<Variant> v; add_rows(v); return v; }();
    for (const Variant& v : variants) {
        if (v.c == d.c && v.ci == d.ci && v.pxt == (wide ? 2 : 1) && v.next == next && v.dw == (d.t1 != nullptr ? 1 : 0)) return v.launch(p, stream);
    }
    // (not reached: the checks above have asked dcb_nsplit_dw_supported / _fin_supported, which read the same table)
    throw std::invalid_argument("dcb_nsplit: no instantiation for this shape, NEXT slot " + std::to_string(next));
}

}  // namespace dcvc
