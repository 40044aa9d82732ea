// fmi_dev_reduce_tree_mx_sr at FMI_F4E2M1, P = 2..16 (fmi_mxfp4_sr_impl.h): the fused stochastic-rounding MXFP4 kernels
// of the left-to-right chain.
#include "fmi_mxfp4_sr_impl.h"

namespace fmi::dev {
template Mxfp4SrUnit mxfp4_sr_unit<sched::kReduceLtr>;
}  // namespace fmi::dev
