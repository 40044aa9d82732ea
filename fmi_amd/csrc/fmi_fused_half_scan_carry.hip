// The carry blocks of scan_no_order beyond 16 peers (sched::kScanCarry, fmi_fused_scan.hip) for the 16-bit float
// dtypes.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kScanCarry, kFusedHalf, 2, sched::kMaxFusedPeers>;
}  // namespace fmi::dev
