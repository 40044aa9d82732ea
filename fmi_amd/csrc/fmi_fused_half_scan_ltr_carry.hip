// The carry blocks of scan_ltr beyond 16 peers (sched::kScanLtrCarry, fmi_fused_scan.hip) for the 16-bit float
// dtypes.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kScanLtrCarry, kFusedHalf, 2, sched::kMaxFusedPeers>;
}  // namespace fmi::dev
