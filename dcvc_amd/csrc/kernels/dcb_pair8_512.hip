// dcb_pair8_kernel.h (adaptor + dc.0 of a block in one launch) instantiated for the 512-wide blocks
#include "dcb_pair8_kernel.h"

namespace dcvc {
namespace pair8 {

template void run_pair<256, 512, 512>(const PairParams&, bool, hipStream_t);
template void run_pair<512, 512, 512>(const PairParams&, bool, hipStream_t);
template void run_pair<192, 512, 512>(const PairParams&, bool, hipStream_t);
template void run_pair<192, 512, 256>(const PairParams&, bool, hipStream_t);

}  // namespace pair8
}  // namespace dcvc
