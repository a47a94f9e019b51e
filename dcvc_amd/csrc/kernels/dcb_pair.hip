// Host side of dcb_pair8_kernel.h: shape dispatch over ADAPTOR_SHAPES (dcb_shapes.h). The adaptor's weight stream is packed with
// the block's other layers in dcb_nsplit.hip. (Includes no kernel: the instantiations live in dcb_pair8_<C>.hip.)
#include "dcb_shapes.h"

namespace dcvc {

namespace {

using pair8::ADAPTOR_SHAPES;
using pair8::N_ADAPTOR_SHAPES;
using RunPair = void (*)(const pair8::PairParams&, bool, hipStream_t);

// (every row's run_pair is named here, so each must exist in some dcb_pair8_<C>.hip: dcb_shapes.h)
template <int I>
RunPair pick_pair(int cin, int c, int ci)
{
    if constexpr (I < N_ADAPTOR_SHAPES) {
        constexpr pair8::AdaptorShape S = ADAPTOR_SHAPES[I];
        if (cin == S.cin && c == S.c && ci == S.ci) return &pair8::run_pair<S.cin, S.c, S.ci>;
        return pick_pair<I + 1>(cin, c, ci);
    }
    return nullptr;
}

}  // namespace

bool dcb_pair_supported(int cin, int c, int ci)
{
    static const bool off = [] { const char* e = getenv("DCVC_PAIR"); return e != nullptr && atoi(e) == 0; }();    // A/B: adaptor and dc.0 as two launches
    if (off) return false;
    for (const pair8::AdaptorShape& s : ADAPTOR_SHAPES)
        if (s.cin == cin && s.c == c && s.ci == ci) return true;
    return false;
}

void dcb_pair(const DcbPairDesc& d, hipStream_t stream)
{
    if (!dcb_pair_supported(d.cin, d.c, d.ci)) throw std::invalid_argument("dcb_pair: no kernel for this (input, block, inner) width");
    if (d.pixels <= 0) throw std::invalid_argument("dcb_pair: empty problem");
    if ((d.ldx % 8) || (d.ldy % 8) || (d.ldt1 % 8)) throw std::invalid_argument("dcb_pair: leading dimensions must be multiples of 8 channels");
    if (!d.x || !d.wa || !d.ba || !d.w1 || !d.b1 || !d.y || !d.t1) throw std::invalid_argument("dcb_pair: missing operand");
    pair8::PairParams p{};
    p.x = d.x; p.ldx = d.ldx; p.wa = reinterpret_cast<const half8*>(d.wa); p.w1 = reinterpret_cast<const half8*>(d.w1);
    p.ba = d.ba; p.b1 = d.b1; p.wsilu = wsilu_table_device();
    p.y = d.y; p.ldy = d.ldy; p.t1 = d.t1; p.ldt1 = d.ldt1; p.M = d.pixels;
    // as the block kernel: 64-pixel workgroups when they fill the chip (run_pair: where the shape has them). DCVC_NSPLIT_PX=32 is
    // the block kernel's A/B switch alone: this launch has never followed it
    const bool wide = d.pixels >= DCB_WIDE_PIXELS;
    pick_pair<0>(d.cin, d.c, d.ci)(p, wide, stream);
}

}  // namespace dcvc
