// decode_kernel_exact.hip -- the exact-shape twins of the north-star decode kernel (decode_kernel.h CTC_EXACT_SHAPES): one
// instantiation per listed shape, in a translation unit of their own so that the units of CTC_KERNEL_LIST stay as they are.
#include "decode_kernel.h"

namespace ctcdk {

#define CTC_X_EXACT_INST(CODE_, K_, V_, BLANK_, LIVE_) template __global__ void ctc_beam_decode_kernel<CODE_, 0, 1, false, 1024, 0, false>(KernelArgs);
CTC_EXACT_SHAPES(CTC_X_EXACT_INST)
#undef CTC_X_EXACT_INST

}  // namespace ctcdk
