// One-pass left-to-right chains beyond 31 peers (P <= 128 per launch; longer chains run as segments of 127
// peers continued from the previous segment's running value, fmi_dev.hip chain_superblocks): scan_ltr (reference PeerToPeer::scan_ltr,
// src/comm/PeerToPeer.cpp:141-152: peer k combines f(prefix of k-1, own)) and reduce_ltr (:44-57: the root
// folds the gathered buckets ((x0 + x1) + x2) + ..). The blocked launches (fmi_dev.hip) run 15 peers at a
// time from a carry bucket; here one thread carries the running value in registers through all P peers,
// 16 loads in flight per step of the runtime block loop. Same operand order, so the same bits; P (+P) bucket
// passes instead of P + 2 ceil((P - 16) / 15) (+P).
#include "fmi_chain_impl.h"

namespace fmi::dev {

int launch_chain_one_pass(int op, int dtype, bool scan, int P, const BlockedScanPtrs& ptrs, size_t n, hipStream_t s,
                          bool carry_in) {
    if (P < 2 || P > kMaxOnePassScanBlocks * BL)
        return fail(FMI_ERR_INVALID, "one-pass chain needs 2 <= P <= " + std::to_string(kMaxOnePassScanBlocks * BL));
    if (is_half_dtype(dtype)) return launch_chain_one_pass_half(op, dtype, scan, P, ptrs, n, s, carry_in);
    return launch_chain_tier<kTierCore>(op, dtype, scan, P, ptrs, n, s, carry_in);
}

}  // namespace fmi::dev
