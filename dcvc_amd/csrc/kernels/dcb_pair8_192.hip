// dcb_pair8_kernel.h (adaptor + dc.0 of a block in one launch) instantiated for the 192-wide block (the intra decoder's last)
#include "dcb_pair8_kernel.h"

namespace dcvc {
namespace pair8 {

template void run_pair<384, 192, 192>(const PairParams&, bool, hipStream_t);

}  // namespace pair8
}  // namespace dcvc
