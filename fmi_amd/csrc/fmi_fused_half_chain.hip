// The one-pass left-to-right chains (fmi_fused_chain.hip) for the 16-bit float dtypes.
#include "fmi_chain_impl.h"

namespace fmi::dev {
int launch_chain_one_pass_half(int op, int dtype, bool scan, int P, const BlockedScanPtrs& ptrs, size_t n, hipStream_t s,
                               bool carry_in) {
    return launch_chain_tier<kTierHalf>(op, dtype, scan, P, ptrs, n, s, carry_in);
}
}  // namespace fmi::dev
