// FMI_ACC_F32 for the 16-bit float dtypes, sum and prod, P = 2..16: the fused kernels of
// allreduce_no_order (fmi_fused_allreduce.hip). Sum and prod give every rank the same bits, so there is
// no rank-selecting form: rank 0's expression serves every rank.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kAllreduce, kFusedAcc32, 2, sched::kMaxFusedPeers>;
}  // namespace fmi::dev
