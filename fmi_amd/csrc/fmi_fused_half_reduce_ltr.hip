// The fused reduce_ltr kernels (fmi_fused_reduce.hip) for the 16-bit float dtypes, P = 2..16.
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_half_reduce_ltr(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    return launch_fused<sched::kReduceLtr, false, 2, sched::kMaxFusedPeers, kTierHalf>(op, dtype, P, ptrs, n, 0, s);
}
}  // namespace fmi::dev
