// The fused scan_ltr kernels for P = 17..31 (fmi_fused_scan_wide.hip) for the 16-bit float dtypes.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kScanLtr, kFusedHalf, sched::kMaxFusedPeers + 1, sched::kMaxFusedScanPeers>;
}  // namespace fmi::dev
