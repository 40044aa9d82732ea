// The one-pass blocked reduce (17..128 peers) and allreduce (P = 32, 64, 128) of fmi_fused_tree_blocked.hip for the
// 16-bit float dtypes.
#include "fmi_tree_blocks_impl.h"

namespace fmi::dev {
int launch_tree_blocks_one_pass_half(int op, int dtype, int alg, int P, const BlockedScanPtrs& ptrs, size_t n, int rank,
                                     hipStream_t s) {
    return launch_tree_blocks_tier<kTierHalf>(op, dtype, alg, P, ptrs, n, rank, s);
}
}  // namespace fmi::dev
