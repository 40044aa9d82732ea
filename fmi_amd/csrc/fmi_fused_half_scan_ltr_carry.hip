// The carry blocks of scan_ltr beyond 16 peers (sched::kScanLtrCarry, fmi_fused_scan.hip) for the 16-bit float
// dtypes.
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_half_scan_ltr_carry(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    return launch_fused<sched::kScanLtrCarry, false, 2, sched::kMaxFusedPeers, kTierHalf>(op, dtype, P, ptrs, n, 0, s);
}
}  // namespace fmi::dev
