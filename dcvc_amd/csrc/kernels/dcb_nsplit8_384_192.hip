// dcb_nsplit8_kernel.h instantiated for the (384, 192) blocks - the low-delay model's prior fusion at picture resolution / 16
// (round 6; one translation unit per block shape)
#include "dcb_nsplit8_kernel.h"

namespace dcvc {
namespace nsplit8 {

template void launch8<384, 192, 1, 0>(const NsParams&, hipStream_t);
template void launch8<384, 192, 2, 0>(const NsParams&, hipStream_t);
template void launch8<384, 192, 1, 1>(const NsParams&, hipStream_t);
template void launch8<384, 192, 2, 1>(const NsParams&, hipStream_t);

}  // namespace nsplit8
}  // namespace dcvc
