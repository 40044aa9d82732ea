// fmi_dev_reduce_tree_mx_sr at the two 8-bit floats, P = 2..16 (fmi_mx_impl.h, SR): the fused stochastic-rounding MX
// kernels of the left-to-right chain.
#include "fmi_mx_impl.h"

namespace fmi::dev {
template MxUnit mx_unit<sched::kReduceLtr, true>;
}  // namespace fmi::dev
