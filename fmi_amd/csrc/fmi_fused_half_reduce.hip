// The fused reduce_no_order kernels (fmi_fused_reduce.hip) for the 16-bit float dtypes, P = 2..16. reduce_ltr and
// reduce-partials stay on the stepwise path for these dtypes (fused_covers).
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_half_reduce(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    return launch_fused<sched::kReduce, false, 2, sched::kMaxFusedPeers, kTierHalf>(op, dtype, P, ptrs, n, 0, s);
}
}  // namespace fmi::dev
