// The one-pass pre-fold allreduce (P = 48, 80, 96, 112) of fmi_fused_tree_blocked.hip for the 16-bit float dtypes.
#include "fmi_tree_blocks_impl.h"

namespace fmi::dev {
int launch_prefold_blocks_one_pass_half(int op, int dtype, int P, const BlockedScanPtrs& ptrs, size_t n, int rank_hi,
                                        hipStream_t s) {
    return launch_prefold_blocks_tier<kTierHalf>(op, dtype, P, ptrs, n, rank_hi, s);
}
}  // namespace fmi::dev
