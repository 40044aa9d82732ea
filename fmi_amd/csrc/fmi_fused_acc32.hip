// Where launch_fused sends a launch whose dtype carries FMI_ACC_F32: the translation unit that holds the family's
// instantiations (fmi_fused_acc32_*.hip, one per family so they build in parallel). The six programs the entry
// points and the communicator's shard step use; everything else (P > 16, unaligned buckets) runs as widen, the f32
// program, narrow (fmi_dev.hip).
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_acc32(int alg, int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    const int st = storage_dtype(dtype);
    switch (alg) {
        case sched::kAllreduce: return launch_fused_acc32_allreduce(op, st, P, ptrs, n, s);
        case sched::kReduce: return launch_fused_acc32_reduce(op, st, P, ptrs, n, s);
        case sched::kReduceLtr: return launch_fused_acc32_reduce_ltr(op, st, P, ptrs, n, s);
        case sched::kReducePartials: return launch_fused_acc32_reduce_partials(op, st, P, ptrs, n, s);
        case sched::kScan: return launch_fused_acc32_scan(op, st, P, ptrs, n, s);
        case sched::kScanLtr: return launch_fused_acc32_scan_ltr(op, st, P, ptrs, n, s);
        default: return fail(FMI_ERR_INVALID, "no f32-accumulating fused kernel for algorithm " + std::to_string(alg));
    }
}
}  // namespace fmi::dev
