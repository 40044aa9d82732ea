// FMI_ACC_F32 for the 16-bit float dtypes, sum and prod, P = 2..16: the fused kernels of
// reduce_no_order (fmi_fused_reduce.hip), inputs in transformed order.
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_acc32_reduce(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    return launch_fused_acc32_family<sched::kReduce>(op, dtype, P, ptrs, n, s);
}
}  // namespace fmi::dev
