// The fused reduce_no_order kernels that store every peer's partial (fmi_fused_reduce.hip) for the 16-bit float
// dtypes, P = 2..16.
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_half_reduce_partials(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    return launch_fused<sched::kReducePartials, false, 2, sched::kMaxFusedPeers, kTierHalf>(op, dtype, P, ptrs, n, 0, s);
}
}  // namespace fmi::dev
