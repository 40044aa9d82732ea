// The one-pass blocked scan (fmi_fused_scan_blocked.hip) over 5..8 full blocks of 16 peers for the 16-bit float
// dtypes.
#include "fmi_fused_impl.h"
#include "fmi_scan_blocks_impl.h"

namespace fmi::dev {
int launch_scan_blocks_one_pass_half_wide(int op, int dtype, int B, const BlockedScanPtrs& ptrs, size_t n, hipStream_t s) {
    return scan_blocks::launch_range<kOnePassScanBlocksNarrow + 1, kMaxOnePassScanBlocks, kTierHalf>(op, dtype, B, ptrs, n, s);
}
}  // namespace fmi::dev
