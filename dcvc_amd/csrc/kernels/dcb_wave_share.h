// dcb_wave_share.h - which of a workgroup's eight waves owns which 32-channel tiles of a layer. THE one statement of the rule: the
// block kernels (dcb_nsplit8_kernel.h, dcb_pair8_kernel.h) consume per-wave weight streams in this order, the host code
// (dcb_nsplit.hip, dcb_pair.hip) packs and sizes them by it. Plain constexpr C++: no HIP calls, any compiler can include it.
//
// Waves w and w + 4 share a SIMD. A layer of n output channels has n / 32 tiles; the waves 0 .. 3 own `hi` tiles each, the waves
// 4 .. 7 `lo` each. Two rules, NOT interchangeable (the tile order differs):
//   by SIMD pair  (n a multiple of 128) a pair owns n / 128 consecutive tiles: wave w the first half rounded up, wave w + 4 the rest
//   by wave       waves 0 .. 3 own ceil(tiles / 8) consecutive tiles each, then the first `act` of the waves 4 .. 7 `lo` each; a wave
//                 behind those has no share: its slots in a packed stream hold tiles of ZEROS (one barrier sequence, one ring discipline)
// A chain-closing conv is always shared by wave; a block's own layers (dc.0, dc.3, ffn.2, the adaptor) by pair where the width
// allows it and by wave otherwise (192). ffn.0's 4 CI channels go in PAIRS of tiles (a pair = 16 channels of t) by the by-wave rule.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCB_SHARE_HD __host__ __device__
#else
#define DCB_SHARE_HD
#endif

namespace dcvc {
namespace nsplit {

struct WaveShare {
    int tiles;          // n / 32
    int hi, lo;         // tiles of each of the waves 0 .. 3 / 4 .. 7
    int act;            // how many of the waves 4 .. 7 have a share
    bool by_pair;

    static DCB_SHARE_HD constexpr WaveShare by_simd_pair(int n) { return WaveShare{n / 32, (n / 128 + 1) / 2, n / 128 / 2, 4, true}; }
    static DCB_SHARE_HD constexpr WaveShare by_wave(int n)
    {
        const int tn = n / 32, hi = (tn + 7) / 8, rem = tn - 4 * hi, lo = rem <= 0 ? 0 : (rem + 3) / 4;
        return WaveShare{tn, hi, lo, lo == 0 ? 0 : rem / lo, false};
    }
    // a layer of a block: dc.0 (n = inner width), dc.3 / ffn.2 / the adaptor (n = block width)
    static DCB_SHARE_HD constexpr WaveShare block_layer(int n) { return n % 128 == 0 ? by_simd_pair(n) : by_wave(n); }

    DCB_SHARE_HD constexpr int tiles_of(bool upper) const { return upper ? lo : hi; }         // upper = a wave 4 .. 7
    // first tile of wave `w` (0 .. 7) and whether it has a share at all
    DCB_SHARE_HD constexpr int first_tile(int w) const
    {
        return by_pair ? (w & 3) * (hi + lo) + (w < 4 ? 0 : hi) : w < 4 ? w * hi : 4 * hi + (w - 4) * lo;
    }
    DCB_SHARE_HD constexpr bool on(int w) const { return by_pair || w < 4 || w - 4 < act; }
    // fragment slots of the packed stream per k-slice of 16, the zero tiles of waves without a share included
    DCB_SHARE_HD constexpr int slots() const { return 4 * (hi + lo); }
    DCB_SHARE_HD constexpr bool even() const { return hi == lo && act == 4; }                 // every wave the same share
    DCB_SHARE_HD constexpr bool covers(int n) const { return n % 32 == 0 && n >= 128 && 4 * hi + act * lo == tiles; }   // the shares add up to the layer
};

// ffn.0: CI / 16 pairs of tiles; the waves 0 .. 3 own `hi` pairs each, 4 .. 7 `lo` (equal but for CI = 192: 2 | 1)
struct Ffn0Share {
    int hi, lo;
    DCB_SHARE_HD constexpr explicit Ffn0Share(int ci) : hi((ci / 16 + 7) / 8), lo((ci / 16 - 4 * ((ci / 16 + 7) / 8)) / 4) {}
    DCB_SHARE_HD constexpr int pairs_of(bool upper) const { return upper ? lo : hi; }
    DCB_SHARE_HD constexpr int first_tile(int w) const { return w < 4 ? 2 * w * hi : 2 * (4 * hi + (w - 4) * lo); }
    DCB_SHARE_HD constexpr bool covers(int ci) const { return ci % 64 == 0 && 4 * (hi + lo) == ci / 16 && lo >= 1; }
};

// the widths in use, spelled out: hi | lo, active upper waves
constexpr bool share_is(WaveShare s, int hi, int lo, int act) { return s.hi == hi && s.lo == lo && s.act == act; }
static_assert(share_is(WaveShare::by_wave(128), 1, 0, 0) && share_is(WaveShare::by_wave(192), 1, 1, 2), "by wave: 128 -> 1 | 0; 192 -> 1 | 1, two active");
static_assert(share_is(WaveShare::by_wave(256), 1, 1, 4) && share_is(WaveShare::by_wave(384), 2, 1, 4), "by wave: 256 -> 1 | 1; 384 -> 2 | 1");
static_assert(share_is(WaveShare::by_wave(512), 2, 2, 4) && share_is(WaveShare::by_wave(768), 3, 3, 4), "by wave: 512 -> 2 | 2; 768 -> 3 | 3");
static_assert(share_is(WaveShare::by_simd_pair(128), 1, 0, 4) && share_is(WaveShare::by_simd_pair(256), 1, 1, 4), "by pair: 128 -> 1 | 0; 256 -> 1 | 1");
static_assert(share_is(WaveShare::by_simd_pair(384), 2, 1, 4) && share_is(WaveShare::by_simd_pair(512), 2, 2, 4), "by pair: 384 -> 2 | 1; 512 -> 2 | 2");
static_assert(share_is(WaveShare::by_simd_pair(768), 3, 3, 4), "by pair: 768 -> 3 | 3");
static_assert(!WaveShare::block_layer(192).by_pair && WaveShare::block_layer(384).by_pair, "a block layer: by pair where n % 128 == 0");
// the two rules order the tiles differently: width 256, wave 1 starts at tile 1 by wave and at tile 2 by pair; wave 4 at 4 and at 1
static_assert(WaveShare::by_wave(256).first_tile(1) == 1 && WaveShare::by_simd_pair(256).first_tile(1) == 2, "tile order");
static_assert(WaveShare::by_wave(256).first_tile(4) == 4 && WaveShare::by_simd_pair(256).first_tile(4) == 1, "tile order");
static_assert(WaveShare::by_wave(192).on(5) && !WaveShare::by_wave(192).on(6) && WaveShare::by_wave(192).slots() == 8, "192: waves 6, 7 idle, eight slots");
static_assert(Ffn0Share(128).hi == 1 && Ffn0Share(128).lo == 1 && Ffn0Share(192).hi == 2 && Ffn0Share(192).lo == 1 && Ffn0Share(256).hi == 2 && Ffn0Share(256).lo == 2, "ffn.0 pairs");
static_assert(Ffn0Share(384).hi == 3 && Ffn0Share(384).lo == 3 && Ffn0Share(512).hi == 4 && Ffn0Share(512).lo == 4 && Ffn0Share(768).hi == 6 && Ffn0Share(768).lo == 6, "ffn.0 pairs");

}  // namespace nsplit
}  // namespace dcvc
