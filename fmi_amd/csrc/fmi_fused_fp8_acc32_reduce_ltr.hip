// FMI_ACC_F32 for the 8-bit float dtypes, P = 2..16 (fmi_fp8_impl.h): the fused kernels of
// reduce_ltr; sum, prod and the mean (FMI_OP_AVG).
#include "fmi_fp8_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kReduceLtr, kFusedFp8Acc32, 2, sched::kMaxFusedPeers>;
}  // namespace fmi::dev
