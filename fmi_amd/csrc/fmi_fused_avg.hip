// Where launch_fused sends a launch with FMI_OP_AVG: the translation unit that holds the algorithm's instantiations
// (fmi_fused_avg_*.hip, one per algorithm so they build in parallel). Only the three reduce algorithms have a mean;
// everything else a mean call can be (P > 16, unaligned buckets) runs the SUM program and then the scale kernel
// (fmi_scale.hip) on its result (fmi_dev.hip).
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_avg(int alg, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    switch (alg) {
        case sched::kAllreduce: return launch_fused_avg_allreduce(dtype, P, ptrs, n, s);
        case sched::kReduce: return launch_fused_avg_reduce(dtype, P, ptrs, n, s);
        case sched::kReduceLtr: return launch_fused_avg_reduce_ltr(dtype, P, ptrs, n, s);
        default: return fail(FMI_ERR_INVALID, "FMI_OP_AVG: no mean for algorithm " + std::to_string(alg) +
                                                  " (only a reduction result has one)");
    }
}
}  // namespace fmi::dev
