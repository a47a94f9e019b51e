// dcb_shapes.h - THE list of shapes the two block kernels are built for. Everything that asks "is there a kernel for this?"
// (dcb_nsplit_shape, dcb_nsplit_fin_supported, dcb_nsplit_dw_supported, dcb_pair_supported, the text of the refusal) and the
// dispatch in dcb_nsplit() / dcb_pair() walk these tables; nothing else names a shape but the instantiation units.
//
// A new shape is a row here plus its explicit instantiations in a unit of its own (dcb_nsplit8_<C>_<CI>[_dw][_fin].hip,
// dcb_pair8_<C>.hip). The dispatch takes the address of every row's launch function, so a row without its instantiation is an
// undefined symbol when the library is linked into the dcvc tool or loaded - not an error at the first call.
#pragma once
#include "dcb_nsplit_common.h"

namespace dcvc {
namespace nsplit8 {

enum class DwInside { none, any_px, px32 };      // the block's depthwise conv inside the launch: never, at either workgroup size, 32-pixel workgroups only

struct BlockShape {
    int c, ci;             // block width, inner width (cdc = cffn)
    int fins[3];           // widths of a chain-closing conv in the NEXT slot (0: unused entry)
    DwInside dw;
    bool px64;             // 64-pixel workgroups exist (768-wide blocks have LDS for 32 pixels only)
};

constexpr BlockShape BLOCK_SHAPES[] = {
    {256, 256, {192}, DwInside::none, true},
    {384, 384, {}, DwInside::none, true},
    {512, 512, {256, 512}, DwInside::none, true},
    {768, 768, {768}, DwInside::none, false},              // the hierarchical models' prior fusion at / 16
    {512, 256, {}, DwInside::none, true},                  // the half-width `dcb2` blocks of the inter models
    {256, 128, {128, 192, 256}, DwInside::any_px, true},   // ... (LDS has room for dc.0's output around a tile only in the narrow blocks)
    {384, 192, {384}, DwInside::px32, true},               // the LD model's prior fusion blocks
    {192, 192, {}, DwInside::none, true},                  // the intra decoder's last block
};
constexpr int N_BLOCK_SHAPES = sizeof(BLOCK_SHAPES) / sizeof(BLOCK_SHAPES[0]);

constexpr const BlockShape* find_block(int c, int ci)
{
    for (const BlockShape& s : BLOCK_SHAPES)
        if (s.c == c && s.ci == ci) return &s;
    return nullptr;
}
constexpr bool has_fin(const BlockShape& s, int nn) { return nn != 0 && (s.fins[0] == nn || s.fins[1] == nn || s.fins[2] == nn); }

// defined in dcb_nsplit8_kernel.h. This one declaration stands for the `extern template` lists: code that includes only this header
// refers to an instantiation without making one
template <int C, int CI, int PXT, int NEXT, int DW = 0>
void launch8(const nsplit::NsParams& p, hipStream_t stream);

}  // namespace nsplit8

namespace pair8 {

struct PairParams {
    const half_t* x; int ldx;        // [M][ldx], first CIN channels
    const half8* wa;                 // packed adaptor weights (dcb_pair_pack_adaptor)
    const half8* w1;                 // packed dc.0 weights (dcb_nsplit_pack_dc0 of the block)
    const half_t* ba; const half_t* b1;
    const float4* wsilu;
    half_t* y; int ldy;              // `in` [M][ldy], C channels
    half_t* t1; int ldt1;            // dc.0 output [M][ldt1], CI channels
    int M;
};

struct AdaptorShape { int cin, c, ci; };      // adaptor input width in front of a (c, ci) block

constexpr AdaptorShape ADAPTOR_SHAPES[] = {
    {448, 256, 128}, {512, 256, 128}, {192, 256, 128},     // LD: encoder, decoder / adaptor_m / spatial prior, adaptor_i
    {128, 256, 256}, {512, 256, 256},                      // intra hyper decoder; hierarchical reconstruction heads
    {192, 384, 384},                                       // intra encoder
    {384, 192, 192},                                       // intra decoder's last block
    {256, 512, 512}, {512, 512, 512}, {192, 512, 512},     // prior fusion, spatial prior adaptors, HT-L adaptor_i
    {192, 512, 256},                                       // HT-S adaptor_i
};
constexpr int N_ADAPTOR_SHAPES = sizeof(ADAPTOR_SHAPES) / sizeof(ADAPTOR_SHAPES[0]);

// defined in dcb_pair8_kernel.h (64-pixel workgroups where the shape's LDS image allows them)
template <int CIN, int C, int CI>
void run_pair(const PairParams& p, bool wide, hipStream_t stream);

}  // namespace pair8
}  // namespace dcvc
