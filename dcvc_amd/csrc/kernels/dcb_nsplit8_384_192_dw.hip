// dcb_nsplit8_kernel.h for the (384, 192) blocks - the LD model's prior fusion at picture resolution / 16 - WITH their depthwise
// conv inside the launch (DW = 1; round 6). 32-pixel workgroups only: with 64 pixels LDS has no room for dc.0's output around a tile.
// (a translation unit of its own: the fully unrolled kernels take minutes to compile, the build runs the units in parallel)
#include "dcb_nsplit8_kernel.h"

namespace dcvc {
namespace nsplit8 {

template void launch8<384, 192, 1, 0, 1>(const NsParams&, hipStream_t);
template void launch8<384, 192, 1, 1, 1>(const NsParams&, hipStream_t);
template void launch8<384, 192, 1, 384, 1>(const NsParams&, hipStream_t);

}  // namespace nsplit8
}  // namespace dcvc
