// One-pass tree reductions beyond the fused kernels, up to 128 peers (blocks of 16 peers):
// reduce_no_order (reference src/comm/PeerToPeer.cpp:59-84; any 17..128 peers, ragged last block included,
// reduce_any_kernel below), allreduce_no_order (:96-130) for
// P = 32, 64, 128 (no pre-fold) and, in prefold_blocks_kernel, P = 48, 80, 96, 112 (whole blocks pre-fold).
// tree_blocked (fmi_dev.hip) evaluates the same bracketing as a launch per block, each writing its block value
// to a temp, then a launch over the B temps: P + 2 B + 1 bucket passes. Here one thread computes its lane
// group's block values in registers and then the block-level program: P + 1 passes. Same programs, same
// operand order, so the same bits.
//   reduce:     binomial rounds 0..3 stay inside each block (the block's 16-peer reduce program); rounds 4..
//               combine the block values at spans 16, 32, ..: the reduce program over the B values.
//   allreduce:  recursive-doubling rounds 0..3 give position p the block's 16-peer allreduce for rank p % 16;
//               rounds 4.. pair positions with equal p % 16: the allreduce program over B values for rank
//               p / 16. Where the bits depend on the rank (float max / min on ±0 / NaN) each block keeps the
//               value of rank % 16 and the block level that of rank / 16 (pick_rank, as the fused kernels);
//               otherwise rank 0's expression is every rank's.
#include "fmi_tree_blocks_impl.h"

namespace fmi::dev {

bool tree_blocks_one_pass_covers(int op, int dtype, int alg, int P) {
    if (alg == FMI_ALG_REDUCE) return P > sched::kMaxFusedPeers && P <= kMaxOnePassScanBlocks * BL;
    if (alg != FMI_ALG_ALLREDUCE || P % BL != 0) return false;
    const int B = P / BL;
    return B >= 2 && B <= kMaxOnePassScanBlocks && (B & (B - 1)) == 0;
}

int launch_tree_blocks_one_pass(int op, int dtype, int alg, int P, const BlockedScanPtrs& ptrs, size_t n, int rank,
                                hipStream_t s) {
    if (!tree_blocks_one_pass_covers(op, dtype, alg, P))
        return fail(FMI_ERR_INVALID, "one-pass blocked tree: unsupported (alg, P, op, dtype)");
    if (is_half_dtype(dtype)) return launch_tree_blocks_one_pass_half(op, dtype, alg, P, ptrs, n, rank, s);
    return launch_tree_blocks_tier<kTierCore>(op, dtype, alg, P, ptrs, n, rank, s);
}

bool prefold_blocks_one_pass_covers(int alg, int P) {
    if (alg != FMI_ALG_ALLREDUCE || P > kMaxOnePassScanBlocks * BL) return false;
    const int pow2 = 1 << sched::floor_log2(P);
    const int folded = P - pow2;
    return (pow2 == 32 || pow2 == 64) && folded > 0 && folded % BL == 0;
}

int launch_prefold_blocks_one_pass(int op, int dtype, int P, const BlockedScanPtrs& ptrs, size_t n, int rank_hi,
                                   hipStream_t s) {
    if (!prefold_blocks_one_pass_covers(FMI_ALG_ALLREDUCE, P))
        return fail(FMI_ERR_INVALID, "one-pass pre-fold allreduce: unsupported P = " + std::to_string(P));
    if (is_half_dtype(dtype)) return launch_prefold_blocks_one_pass_half(op, dtype, P, ptrs, n, rank_hi, s);
    return launch_prefold_blocks_tier<kTierCore>(op, dtype, P, ptrs, n, rank_hi, s);
}

}  // namespace fmi::dev
