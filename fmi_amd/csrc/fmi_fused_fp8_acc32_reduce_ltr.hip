// FMI_ACC_F32 for the 8-bit float dtypes, P = 2..16 (fmi_fp8_impl.h): the fused kernels of
// reduce_ltr; sum, prod and the mean (FMI_OP_AVG).
#include "fmi_fp8_impl.h"

namespace fmi::dev {
int launch_fused_fp8_acc32_reduce_ltr(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    return launch_fused_fp8_acc32_family<sched::kReduceLtr>(op, dtype, P, ptrs, n, s);
}
}  // namespace fmi::dev
