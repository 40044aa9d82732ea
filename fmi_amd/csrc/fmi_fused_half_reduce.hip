// The fused reduce_no_order kernels (fmi_fused_reduce.hip) for the 16-bit float dtypes, P = 2..16. reduce_ltr and
// reduce-partials are in fmi_fused_half_reduce_ltr.hip / _reduce_partials.hip, P > 16 in fmi_fused_half_tree_blocks.hip.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kReduce, kFusedHalf, 2, sched::kMaxFusedPeers>;
}  // namespace fmi::dev
