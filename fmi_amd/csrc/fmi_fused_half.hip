// Where launch_fused's core tier sends a 16-bit float launch: the translation unit that holds the (alg, P)
// instantiations (fmi_fused_half_*.hip, one per family and peer range, so they build in parallel and the core
// units keep their device code).
#include "fmi_fused_impl.h"

namespace fmi::dev {
int launch_fused_half(int alg, bool rank_aware, int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, int rank,
                      hipStream_t s) {
    const bool wide = P > sched::kMaxFusedPeers;
    switch (alg) {
        case sched::kAllreduce:
            if (!wide) return launch_fused_half_allreduce(op, dtype, rank_aware, P, ptrs, n, rank, s);
            return dtype == FMI_F16 ? launch_fused_half_allreduce_wide_f16(op, P, ptrs, n, rank, s)
                                    : launch_fused_half_allreduce_wide_bf16(op, P, ptrs, n, rank, s);
        case sched::kAllreducePrefold16: return launch_fused_half_prefold16(op, dtype, ptrs, n, s);
        case sched::kReduce: return launch_fused_half_reduce(op, dtype, P, ptrs, n, s);
        case sched::kReduceLtr: return launch_fused_half_reduce_ltr(op, dtype, P, ptrs, n, s);
        case sched::kReducePartials: return launch_fused_half_reduce_partials(op, dtype, P, ptrs, n, s);
        case sched::kScan:
            return wide ? launch_fused_half_scan_wide(op, dtype, P, ptrs, n, s) : launch_fused_half_scan(op, dtype, P, ptrs, n, s);
        case sched::kScanLtr:
            return wide ? launch_fused_half_scan_ltr_wide(op, dtype, P, ptrs, n, s)
                        : launch_fused_half_scan_ltr(op, dtype, P, ptrs, n, s);
        case sched::kScanCarry: return launch_fused_half_scan_carry(op, dtype, P, ptrs, n, s);
        case sched::kScanLtrCarry: return launch_fused_half_scan_ltr_carry(op, dtype, P, ptrs, n, s);
        default: return fail(FMI_ERR_INVALID, "no fused kernel for algorithm " + std::to_string(alg));
    }
}
}  // namespace fmi::dev
