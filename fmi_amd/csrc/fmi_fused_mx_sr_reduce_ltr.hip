// fmi_dev_reduce_tree_mx_sr at the two 8-bit floats, P = 2..16 (fmi_mx_sr_impl.h): the fused stochastic-rounding MX
// kernels of the left-to-right chain.
#include "fmi_mx_sr_impl.h"

namespace fmi::dev {
template MxSrUnit mx_sr_unit<sched::kReduceLtr>;
}  // namespace fmi::dev
