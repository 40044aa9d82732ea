// FMI_OP_AVG, P = 2..16: the fused kernels of allreduce_no_order at op OpAvg, for f32, f64, f16, bf16 and the two 16-bit floats
// with f32 values (FMI_ACC_F32). The SUM program with the stored value scaled by fl(1 / P): one launch, P reads, one store.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kAllreduce, kFusedAvg, 2, sched::kMaxFusedPeers>;
}  // namespace fmi::dev
