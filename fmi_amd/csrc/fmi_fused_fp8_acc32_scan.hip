// FMI_ACC_F32 for the 8-bit float dtypes, P = 2..16 (fmi_fp8_impl.h): the fused kernels of
// scan_no_order, every prefix its own f32 value narrowed once; sum and prod.
#include "fmi_fp8_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kScan, kFusedFp8Acc32, 2, sched::kMaxFusedPeers>;
}  // namespace fmi::dev
