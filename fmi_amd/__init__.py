"""fmi_amd — MI355X-native (gfx950) engine for FMI's bucket reduction (reduce / allreduce / scan).

Layout:
  include/fmi_dev.h          C-ABI (the drop-in boundary)
  fmi_amd/csrc/              HIP kernels + C-ABI implementation → fmi_amd/lib/libfmi_dev.so
  fmi_amd/cpp/include/fmi/   C++ mirror of the FMI::Communicator surface (reference include/)
  fmi_amd/device.py          Python handle over the C-ABI (ctypes)
  fmi_amd/collectives.py     multi-GPU sharded allreduce over torch.distributed (RCCL over xGMI)
"""
from ._lib import FmiError, LIB_PATH, Timeout, load  # noqa: F401
from .device import (  # noqa: F401
    ACC_F32, Alg, Bucket, DType, Event, Graph, HostRegistration, Op, PinnedArray, Stream, Tune, combine, convert, describe,
    device_count, finalize, fp4_pack, fp4_unpack, fp6_pack, fp6_unpack, host_reduce_pair, init, mean_scale, mx_blocks, mx_dequantize, mx_quantize, mx_quantize_sr_host, pci_bus_id, reduce_pair, reduce_pair_batch, reduce_tree, reduce_tree_mx, reduce_tree_scaled, scan_peers, schedule_expr, sync, tune_get, tune_set,
)

__all__ = [
    "ACC_F32", "Alg", "Bucket", "DType", "Event", "FmiError", "Graph", "HostRegistration", "LIB_PATH", "Op", "PinnedArray", "Stream",
    "Timeout", "Tune", "combine", "convert", "describe", "device_count", "finalize", "fp4_pack", "fp4_unpack", "fp6_pack", "fp6_unpack", "host_reduce_pair", "init", "load", "mean_scale", "mx_blocks", "mx_dequantize", "mx_quantize", "mx_quantize_sr_host", "pci_bus_id", "reduce_pair", "reduce_pair_batch",
    "reduce_tree", "reduce_tree_mx", "reduce_tree_scaled", "scan_peers", "schedule_expr", "sync", "tune_get", "tune_set",
]
