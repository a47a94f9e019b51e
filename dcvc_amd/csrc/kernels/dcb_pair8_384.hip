// dcb_pair8_kernel.h (adaptor + dc.0 of a block in one launch) instantiated for the 384-wide blocks
#include "dcb_pair8_kernel.h"

namespace dcvc {
namespace pair8 {

template void run_pair<192, 384, 384>(const PairParams&, bool, hipStream_t);

}  // namespace pair8
}  // namespace dcvc
