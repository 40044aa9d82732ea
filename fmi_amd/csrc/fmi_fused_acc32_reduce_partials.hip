// FMI_ACC_F32 for the 16-bit float dtypes, sum and prod, P = 2..16: the fused kernels of
// reduce_no_order with every peer's final sendbuf stored (fmi_fused_reduce.hip): each partial is its own f32
// value, narrowed once.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kReducePartials, kFusedAcc32, 2, sched::kMaxFusedPeers>;
}  // namespace fmi::dev
