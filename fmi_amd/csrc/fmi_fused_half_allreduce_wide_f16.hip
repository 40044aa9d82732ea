// The fused allreduce_no_order kernels for P = 17..31 (fmi_fused_allreduce_wide.hip) for f16: rank 0's form for
// sum / prod, the rank-selecting form for max / min. The largest programs of the half tier, so each of the two
// dtypes builds in a translation unit of its own.
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_half_allreduce_wide_f16(int op, int P, const PeerPtrs& ptrs, size_t n, int rank, hipStream_t s) {
    return launch_fused<sched::kAllreduce, true, sched::kMaxFusedPeers + 1, sched::kMaxFusedAllreducePeers, kTierF16>(
        op, FMI_F16, P, ptrs, n, rank, s);
}
}  // namespace fmi::dev
