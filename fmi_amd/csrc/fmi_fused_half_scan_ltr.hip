// The fused scan_ltr kernels (fmi_fused_scan.hip) for the 16-bit float dtypes, P = 2..16.
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_half_scan_ltr(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    return launch_fused<sched::kScanLtr, false, 2, sched::kMaxFusedPeers, kTierHalf>(op, dtype, P, ptrs, n, 0, s);
}
}  // namespace fmi::dev
