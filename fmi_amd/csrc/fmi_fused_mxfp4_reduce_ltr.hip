// fmi_dev_reduce_tree_mx at FMI_F4E2M1, P = 2..16 (fmi_mxfp4_impl.h): the fused MXFP4 kernels of reduce_ltr, E2M1 and f32
// output.
#include "fmi_mxfp4_impl.h"

namespace fmi::dev {
template MxUnit mxfp4_unit<sched::kReduceLtr, false>;
}  // namespace fmi::dev
