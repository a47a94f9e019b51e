// dcb_nsplit8_kernel.h instantiated for the (192, 192) block - the intra decoder's last block, dec.dec_2 (round 6: block width
// 192 = six tiles on six of the eight waves, LDS rows of both tensors padded to 256 channels)
#include "dcb_nsplit8_kernel.h"

namespace dcvc {
namespace nsplit8 {

template void launch8<192, 192, 1, 0>(const NsParams&, hipStream_t);
template void launch8<192, 192, 2, 0>(const NsParams&, hipStream_t);
template void launch8<192, 192, 1, 1>(const NsParams&, hipStream_t);
template void launch8<192, 192, 2, 1>(const NsParams&, hipStream_t);

}  // namespace nsplit8
}  // namespace dcvc
