// The fused allreduce_no_order kernels for P = 17..31 (fmi_fused_allreduce_wide.hip) for f16: rank 0's form for
// sum / prod, the rank-selecting form for max / min. The largest programs of the half tier, so each of the two
// dtypes builds in a translation unit of its own.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kAllreduce, kFusedF16, sched::kMaxFusedPeers + 1, sched::kMaxFusedAllreducePeers, kRankPicked>;
}  // namespace fmi::dev
