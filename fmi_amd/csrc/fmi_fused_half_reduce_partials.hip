// The fused reduce_no_order kernels that store every peer's partial (fmi_fused_reduce.hip) for the 16-bit float
// dtypes, P = 2..16.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kReducePartials, kFusedHalf, 2, sched::kMaxFusedPeers>;
}  // namespace fmi::dev
