// dcb_nsplit8_kernel.h for the (256, 128) blocks WITH their depthwise conv inside the launch (DW = 1; round 6): the inter models'
// blocks at picture resolution / 8 and / 16 - a launch and a round trip of the 128-channel tensor through memory less per block
// (a translation unit of its own: the fully unrolled kernels take minutes to compile, the build runs the units in parallel)
#include "dcb_nsplit8_kernel.h"

namespace dcvc {
namespace nsplit8 {

template void launch8<256, 128, 1, 0, 1>(const NsParams&, hipStream_t);
template void launch8<256, 128, 2, 0, 1>(const NsParams&, hipStream_t);
template void launch8<256, 128, 1, 1, 1>(const NsParams&, hipStream_t);
template void launch8<256, 128, 2, 1, 1>(const NsParams&, hipStream_t);

}  // namespace nsplit8
}  // namespace dcvc
