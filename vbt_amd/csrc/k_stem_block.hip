// The network entry: stem 3x3/2 + first SeparableConv in one kernel, both forms (stem_block.h).
#include "launchers.h"
#include "stem_block.h"

namespace vbt {

int launch_stem_block(const StemBlockArgs& a, bool direct, unsigned grid, hipStream_t st) {
  const bool full_range = a.rqs.full && a.rqd.full && a.rqp.full;
  const int mode = full_range ? (a.rqs.kb && a.rqd.kb && a.rqp.kb ? 3 : 1) : 0;
  if (direct) {
    if (mode == 3) stem_block_direct_kernel<3><<<dim3(grid), 256, 0, st>>>(a);
    else if (mode == 1) stem_block_direct_kernel<1><<<dim3(grid), 256, 0, st>>>(a);
    else stem_block_direct_kernel<0><<<dim3(grid), 256, 0, st>>>(a);
  } else {
    if (mode == 3) stem_block_kernel<3><<<dim3(grid), 256, 0, st>>>(a);
    else if (mode == 1) stem_block_kernel<1><<<dim3(grid), 256, 0, st>>>(a);
    else stem_block_kernel<0><<<dim3(grid), 256, 0, st>>>(a);
  }
  return VBT_OK;
}

}  // namespace vbt
