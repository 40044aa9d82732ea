// Fused single-pass peer-axis scans in the order of reference PeerToPeer::scan_no_order
// (src/comm/PeerToPeer.cpp:154-184) and PeerToPeer::scan_ltr (src/comm/PeerToPeer.cpp:141-152), P = 2..16, and the
// carry blocks of both beyond 16 peers (sched::kScanCarry / kScanLtrCarry); 17..31 in fmi_fused_scan_wide.hip.
#include "fmi_fused_impl.h"

namespace fmi::dev {
template FusedUnit fused_unit<sched::kScan, kFusedCore, 2, sched::kMaxFusedPeers>;
template FusedUnit fused_unit<sched::kScanLtr, kFusedCore, 2, sched::kMaxFusedPeers>;
template FusedUnit fused_unit<sched::kScanCarry, kFusedCore, 2, sched::kMaxFusedPeers>;
template FusedUnit fused_unit<sched::kScanLtrCarry, kFusedCore, 2, sched::kMaxFusedPeers>;
}  // namespace fmi::dev
