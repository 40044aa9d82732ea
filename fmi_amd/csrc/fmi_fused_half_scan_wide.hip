// The fused scan_no_order kernels for P = 17..31 (fmi_fused_scan_wide.hip) for the 16-bit float dtypes.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kScan, kFusedHalf, sched::kMaxFusedPeers + 1, sched::kMaxFusedScanPeers>;
}  // namespace fmi::dev
