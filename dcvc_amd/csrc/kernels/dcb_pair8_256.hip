// dcb_pair8_kernel.h (adaptor + dc.0 of a block in one launch) instantiated for the 256-wide blocks
#include "dcb_pair8_kernel.h"

namespace dcvc {
namespace pair8 {

template void run_pair<448, 256, 128>(const PairParams&, bool, hipStream_t);
template void run_pair<512, 256, 128>(const PairParams&, bool, hipStream_t);
template void run_pair<192, 256, 128>(const PairParams&, bool, hipStream_t);
template void run_pair<128, 256, 256>(const PairParams&, bool, hipStream_t);
template void run_pair<512, 256, 256>(const PairParams&, bool, hipStream_t);

}  // namespace pair8
}  // namespace dcvc
