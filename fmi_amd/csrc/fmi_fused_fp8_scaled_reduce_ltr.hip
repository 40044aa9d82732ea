// fmi_dev_reduce_tree_scaled, P = 2..16 (fmi_fp8_scaled_impl.h): the fused scaled kernels of reduce_ltr, both 8-bit
// floats, 8-bit and f32 output.
#include "fmi_fp8_scaled_impl.h"

namespace fmi::dev {
template ScaledUnit scaled_unit<sched::kReduceLtr>;
}  // namespace fmi::dev
