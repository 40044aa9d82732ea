// The fused allreduce_no_order kernels (fmi_fused_allreduce.hip) for the 16-bit float dtypes, P = 2..16: the
// rank-0 form (also the P = 2^k pointer permutation's target) and the rank-selecting form for max / min. P = 17..31 in
// fmi_fused_half_allreduce_wide_{f16,bf16}.hip.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kAllreduce, kFusedHalf, 2, sched::kMaxFusedPeers>;
template FusedUnit fused_unit<sched::kAllreduce, kFusedHalf, 2, sched::kMaxFusedPeers, kRankPicked>;
}  // namespace fmi::dev
