// The fused allreduce_no_order kernels (fmi_fused_allreduce.hip) for the 16-bit float dtypes, P = 2..16: the
// rank-0 form (also the P = 2^k pointer permutation's target) and the rank-selecting form for max / min. P = 17..31 in
// fmi_fused_half_allreduce_wide_{f16,bf16}.hip.
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_half_allreduce(int op, int dtype, bool rank_aware, int P, const PeerPtrs& ptrs, size_t n, int rank,
                                hipStream_t s) {
    if (rank_aware) return launch_fused<sched::kAllreduce, true, 2, sched::kMaxFusedPeers, kTierHalf>(op, dtype, P, ptrs, n, rank, s);
    return launch_fused<sched::kAllreduce, false, 2, sched::kMaxFusedPeers, kTierHalf>(op, dtype, P, ptrs, n, rank, s);
}
}  // namespace fmi::dev
