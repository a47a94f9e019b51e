// dcb_nsplit8_kernel.h instantiated for the (512, 256) blocks (one translation unit per block shape: the fully unrolled kernels take minutes to compile, the build runs the units in parallel)
#include "dcb_nsplit8_kernel.h"

namespace dcvc {
namespace nsplit8 {

template void launch8<512, 256, 1, 0>(const NsParams&, hipStream_t);
template void launch8<512, 256, 2, 0>(const NsParams&, hipStream_t);
template void launch8<512, 256, 1, 1>(const NsParams&, hipStream_t);
template void launch8<512, 256, 2, 1>(const NsParams&, hipStream_t);

}  // namespace nsplit8
}  // namespace dcvc
