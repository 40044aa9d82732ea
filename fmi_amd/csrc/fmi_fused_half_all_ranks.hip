// Every peer's value of the allreduce program at once (kRankEvery, fmi_fused_allreduce.hip)
// for the 16-bit float dtypes: max / min keep one operand's bits, so on ±0 ties and NaNs the peers differ.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kAllreduce, kFusedHalf, 2, sched::kMaxFusedPeers, kRankEvery>;
}  // namespace fmi::dev
