// fmi_dev_reduce_tree_mx at FMI_F6E2M3 / FMI_F6E3M2, P = 2..16 (fmi_mxfp6_impl.h): the fused MXFP6 kernels of allreduce,
// FP6 and f32 output.
#include "fmi_mxfp6_impl.h"

namespace fmi::dev {
template MxUnit mxfp6_unit<sched::kAllreduce, false>;
}  // namespace fmi::dev
