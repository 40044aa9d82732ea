// Fused single-pass kernels in the order of reference PeerToPeer::allreduce_no_order
// (src/comm/PeerToPeer.cpp:96-130), P = 2..16; 17..31 in fmi_fused_allreduce_wide.hip. Rank 0's form (also the target
// of the P = 2^k pointer permutation, launch_fused in fmi_fused.hip) and the rank-selecting form for float max / min.
// kRankEvery: every peer's value of the same program at once (ptrs.out[r] = the value peer r holds), for the
// operand-order-sensitive ops only (float max / min): a sharded allreduce hands each rank the shard
// reductions in that rank's own order. One pass: P reads, P writes.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kAllreduce, kFusedCore, 2, sched::kMaxFusedPeers>;
template FusedUnit fused_unit<sched::kAllreduce, kFusedCore, 2, sched::kMaxFusedPeers, kRankPicked>;
template FusedUnit fused_unit<sched::kAllreduce, kFusedCore, 2, sched::kMaxFusedPeers, kRankEvery>;
}  // namespace fmi::dev
