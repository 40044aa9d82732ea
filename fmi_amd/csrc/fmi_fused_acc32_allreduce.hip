// FMI_ACC_F32 for the 16-bit float dtypes, sum and prod, P = 2..16: the fused kernels of
// allreduce_no_order (fmi_fused_allreduce.hip). Sum and prod give every rank the same bits, so there is
// no rank-selecting form and no pointer permutation: rank 0's expression serves every rank.
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_acc32_allreduce(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    return launch_fused_acc32_family<sched::kAllreduce>(op, dtype, P, ptrs, n, s);
}
}  // namespace fmi::dev
