// The fused scan_ltr kernels for P = 17..31 (fmi_fused_scan_wide.hip) for the 16-bit float dtypes.
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_half_scan_ltr_wide(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    return launch_fused<sched::kScanLtr, false, sched::kMaxFusedPeers + 1, sched::kMaxFusedScanPeers, kTierHalf>(op, dtype, P, ptrs, n, 0, s);
}
}  // namespace fmi::dev
