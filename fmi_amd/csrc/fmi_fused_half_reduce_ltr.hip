// The fused reduce_ltr kernels (fmi_fused_reduce.hip) for the 16-bit float dtypes, P = 2..16.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kReduceLtr, kFusedHalf, 2, sched::kMaxFusedPeers>;
}  // namespace fmi::dev
