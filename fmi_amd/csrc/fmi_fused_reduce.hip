// Fused single-pass kernels in the order of reference PeerToPeer::reduce_no_order
// (src/comm/PeerToPeer.cpp:59-84) and PeerToPeer::reduce_ltr (src/comm/PeerToPeer.cpp:44-57); the reduce with
// every peer's final sendbuf as an output (its partial, :72) for the reference-faithful sharded reduce.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kReduce, kFusedCore, 2, sched::kMaxFusedPeers>;
template FusedUnit fused_unit<sched::kReduceLtr, kFusedCore, 2, sched::kMaxFusedPeers>;
template FusedUnit fused_unit<sched::kReducePartials, kFusedCore, 2, sched::kMaxFusedPeers>;
}  // namespace fmi::dev
