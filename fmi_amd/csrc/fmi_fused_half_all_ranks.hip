// Every peer's value of the allreduce program at once (launch_fused_allreduce_all_ranks, fmi_fused_allreduce.hip)
// for the 16-bit float dtypes: max / min keep one operand's bits, so on ±0 ties and NaNs the peers differ.
#include "fmi_fused_impl.h"

namespace fmi::dev {
namespace {
template <class Op, class T, int P>
void all_ranks_one(const PeerPtrs& ptrs, size_t n, int, hipStream_t s) {
    const size_t nvec = n / kVecLanes<T>;
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(grid_for(nvec, kFusedBlock), kFusedGridCap));
    scan_kernel<Op, T, sched::kAllreduce, P><<<grid, kFusedBlock, fused_lds_bytes(P, kFusedBlock * 16), s>>>(ptrs, n, fused_policy(true, P));
}

template <class Op, class T, int... I>
constexpr std::array<FusedFn, sizeof...(I)> all_ranks_table(std::integer_sequence<int, I...>) {
    return {&all_ranks_one<Op, T, I + 2>...};
}
}  // namespace

int launch_fused_half_all_ranks(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    if (P < 2 || P > sched::kMaxFusedPeers)
        return fail(FMI_ERR_INVALID, "all-ranks allreduce kernel needs 2 <= P <= 16, got " + std::to_string(P));
    return with_op_dtype<kTierHalf>(op, dtype, [&]<class Op, class T>() -> int {
        if constexpr (std::is_same_v<Op, OpMax> || std::is_same_v<Op, OpMin>) {
            static constexpr auto table = all_ranks_table<Op, T>(std::make_integer_sequence<int, sched::kMaxFusedPeers - 1>{});
            table[P - 2](ptrs, n, 0, s);
            return check_launch("all-ranks allreduce kernel launch");
        } else {
            return fail(FMI_ERR_INVALID, "all-ranks allreduce kernel: only float max / min depend on the rank");
        }
    });
}
}  // namespace fmi::dev
