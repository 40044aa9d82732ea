// Fused single-pass peer-axis scans for P = 17..31 (reference PeerToPeer::scan_no_order,
// src/comm/PeerToPeer.cpp:154-184, and scan_ltr, :141-152): all P inputs read and all P outputs written in
// one pass. Its own translation unit so these larger programs build in parallel with the rest.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kScan, kFusedCore, sched::kMaxFusedPeers + 1, sched::kMaxFusedScanPeers>;
template FusedUnit fused_unit<sched::kScanLtr, kFusedCore, sched::kMaxFusedPeers + 1, sched::kMaxFusedScanPeers>;
}  // namespace fmi::dev
