// The one-pass blocked scan (fmi_fused_scan_blocked.hip) over 2..4 full blocks of 16 peers for the 16-bit float
// dtypes; 5..8 blocks in fmi_fused_half_scan_blocks_wide.hip.
#include "fmi_fused_impl.h"
#include "fmi_scan_blocks_impl.h"

namespace fmi::dev {
int launch_scan_blocks_one_pass_half(int op, int dtype, int B, const BlockedScanPtrs& ptrs, size_t n, hipStream_t s) {
    if (B > kOnePassScanBlocksNarrow) return launch_scan_blocks_one_pass_half_wide(op, dtype, B, ptrs, n, s);
    return scan_blocks::launch_range<2, kOnePassScanBlocksNarrow, kTierHalf>(op, dtype, B, ptrs, n, s);
}
}  // namespace fmi::dev
