// The fused reduce_no_order kernels (fmi_fused_reduce.hip) for the 16-bit float dtypes, P = 2..16. reduce_ltr and
// reduce-partials are in fmi_fused_half_reduce_ltr.hip / _reduce_partials.hip, P > 16 in fmi_fused_half_tree_blocks.hip.
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_half_reduce(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    return launch_fused<sched::kReduce, false, 2, sched::kMaxFusedPeers, kTierHalf>(op, dtype, P, ptrs, n, 0, s);
}
}  // namespace fmi::dev
