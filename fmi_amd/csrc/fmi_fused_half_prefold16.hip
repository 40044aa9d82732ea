// The 32-input pre-fold block of an allreduce beyond 31 peers (sched::kAllreducePrefold16,
// fmi_fused_allreduce_wide.hip; launch_fused has permuted the pointers by the rank already) for the 16-bit float dtypes.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kAllreducePrefold16, kFusedHalf, 32, 32>;
}  // namespace fmi::dev
