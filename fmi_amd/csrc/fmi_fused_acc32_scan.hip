// FMI_ACC_F32 for the 16-bit float dtypes, sum and prod, P = 2..16: the fused kernels of
// scan_no_order (fmi_fused_scan.hip): each prefix is its own f32 value, narrowed once.
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_acc32_scan(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    return launch_fused_acc32_family<sched::kScan>(op, dtype, P, ptrs, n, s);
}
}  // namespace fmi::dev
