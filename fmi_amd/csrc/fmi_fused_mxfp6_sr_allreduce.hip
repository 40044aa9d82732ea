// fmi_dev_reduce_tree_mx_sr at FMI_F6E2M3 / FMI_F6E3M2, P = 2..16 (fmi_mxfp6_impl.h, SR): the fused stochastic-rounding
// MXFP6 kernels of allreduce.
#include "fmi_mxfp6_impl.h"

namespace fmi::dev {
template MxUnit mxfp6_unit<sched::kAllreduce, true>;
}  // namespace fmi::dev
