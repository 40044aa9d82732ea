// fmi_dev_reduce_tree_mx_sr at FMI_F4E2M1, P = 2..16 (fmi_mxfp4_impl.h, SR): the fused stochastic-rounding MXFP4 kernels
// of the left-to-right chain.
#include "fmi_mxfp4_impl.h"

namespace fmi::dev {
template MxUnit mxfp4_unit<sched::kReduceLtr, true>;
}  // namespace fmi::dev
