// The fused scan_no_order kernels (fmi_fused_scan.hip) for the 16-bit float dtypes, P = 2..16. scan_ltr, the
// carry blocks, P = 17..31 and the one-pass blocked forms each have a unit of their own (fmi_fused_half_scan_*.hip).
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kScan, kFusedHalf, 2, sched::kMaxFusedPeers>;
}  // namespace fmi::dev
