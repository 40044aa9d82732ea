// Where launch_fused sends a launch on 8-bit float buckets (FMI_F8E4M3 / FMI_F8E5M2 with FMI_ACC_F32; op sum, prod or
// FMI_OP_AVG): the translation unit that holds the family's instantiations (fmi_fused_fp8_acc32_*.hip, one per family
// so they build in parallel). Everything else on these dtypes runs elsewhere (fmi_dev.hip): P > 16 and unaligned
// buckets as widen, the f32 program, narrow; the plain dtypes as pairwise passes in the program's order.
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_fp8_acc32(int alg, int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    switch (alg) {
        case sched::kAllreduce: return launch_fused_fp8_acc32_allreduce(op, dtype, P, ptrs, n, s);
        case sched::kReduce: return launch_fused_fp8_acc32_reduce(op, dtype, P, ptrs, n, s);
        case sched::kReduceLtr: return launch_fused_fp8_acc32_reduce_ltr(op, dtype, P, ptrs, n, s);
        case sched::kReducePartials: return launch_fused_fp8_acc32_reduce_partials(op, dtype, P, ptrs, n, s);
        case sched::kScan: return launch_fused_fp8_acc32_scan(op, dtype, P, ptrs, n, s);
        case sched::kScanLtr: return launch_fused_fp8_acc32_scan_ltr(op, dtype, P, ptrs, n, s);
        default: return fail(FMI_ERR_INVALID, "no f32-accumulating fused kernel for algorithm " + std::to_string(alg));
    }
}
}  // namespace fmi::dev
