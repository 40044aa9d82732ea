// The 32-input pre-fold block of an allreduce beyond 31 peers (sched::kAllreducePrefold16,
// fmi_fused_allreduce_wide.hip, which has permuted the pointers by the rank already) for the 16-bit float dtypes.
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_half_prefold16(int op, int dtype, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    return launch_fused<sched::kAllreducePrefold16, false, 32, 32, kTierHalf>(op, dtype, 32, ptrs, n, 0, s);
}
}  // namespace fmi::dev
