// fmi_dev_reduce_tree_mx, P = 2..16 (fmi_mx_impl.h): the fused MX kernels of reduce_no_order, both 8-bit floats, 8-bit and
// f32 output.
#include "fmi_mx_impl.h"

namespace fmi::dev {
template MxUnit mx_unit<sched::kReduce, false>;
}  // namespace fmi::dev
