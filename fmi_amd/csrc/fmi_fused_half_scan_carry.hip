// The carry blocks of scan_no_order beyond 16 peers (sched::kScanCarry, fmi_fused_scan.hip) for the 16-bit float
// dtypes.
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_half_scan_carry(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    return launch_fused<sched::kScanCarry, false, 2, sched::kMaxFusedPeers, kTierHalf>(op, dtype, P, ptrs, n, 0, s);
}
}  // namespace fmi::dev
