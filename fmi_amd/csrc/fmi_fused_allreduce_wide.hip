// Fused single-pass allreduce_no_order (reference src/comm/PeerToPeer.cpp:96-130) for P = 17..31: the
// pre-fold of peers 16.. into peers 0.. (:100-107) and the 16-peer recursive doubling (:108-121) in one pass
// over all P inputs. Its own translation unit: these programs are the largest and build in parallel with
// the rest. And the 32-input pre-fold block of an allreduce beyond 31 peers (sched::kAllreducePrefold16), whose
// pointers launch_fused (fmi_fused.hip) has permuted by the rank.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kAllreduce, kFusedCore, sched::kMaxFusedPeers + 1, sched::kMaxFusedAllreducePeers, kRankPicked>;
template FusedUnit fused_unit<sched::kAllreducePrefold16, kFusedCore, 32, 32>;
}  // namespace fmi::dev
