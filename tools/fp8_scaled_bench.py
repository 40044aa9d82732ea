"""The scaled FP8 kernel (fmi_dev_reduce_tree_scaled) beside the unscaled FMI_F8E4M3 | FMI_ACC_F32 SUM ALLREDUCE kernel,
on one GPU, timed with events, by the protocol of tools/fp8_kernels.py:

  unscaled          reduce_tree SUM ALLREDUCE with accumulate_f32 (the yardstick: its code is not the scaled call's)
  scaled            reduce_tree_scaled, out = the inputs' dtype, amax = NULL
  scaled_amax       the same with amax
  scaled_f32        reduce_tree_scaled, out = F32, amax = NULL

P = 8 peers of 256 MiB each, the inputs (and the 8-bit output) of a set carved as one group (fmi_dev_alloc_group), the f32
output a bucket of its own; three rotating sets, so that no bucket returns within 256 MB of the Infinity Cache; the four
kernels interleaved in one process, three passes. One JSON line per kernel: bytes/s per pass and their median, the
fraction of 8 TB/s (algorithmic bytes: P * n + n * sizeof(out)), the ratio to the yardstick of the same pass, and the
yardstick's own spread over the passes.

    python3 tools/fp8_scaled_bench.py [--kind e4m3] [--label NAME] [--out profiles/fp8_scaled_bench.jsonl]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import fmi_amd  # noqa: E402
from fmi_amd import Alg, Bucket, DType, Op  # noqa: E402
from half_kernels import MIB, PASSES, emit, timed  # noqa: E402

ROWS = ("unscaled", "scaled", "scaled_amax", "scaled_f32")  # the first is the yardstick
PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="e4m3", choices=("e4m3", "e5m2"))
    ap.add_argument("--mib", type=int, default=256, help="bytes per input bucket")
    ap.add_argument("--peers", type=int, default=8)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--iters", type=int, default=24, help="timed launches per kernel and pass")
    ap.add_argument("--inflight-kib", type=int, default=None, help="set FMI_TUNE_FUSED_INFLIGHT_KIB first (0 = no cap)")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    fmi_amd.init(0)
    if args.inflight_kib is not None:
        fmi_amd.tune_set(fmi_amd.Tune.FUSED_INFLIGHT_KIB, args.inflight_kib)
    dt = DType.F8E4M3 if args.kind == "e4m3" else DType.F8E5M2
    P, n = args.peers, args.mib * MIB
    groups = [Bucket.group(P + 1, n, dt) for _ in range(args.sets)]
    wide = [Bucket(n, np.float32) for _ in range(args.sets)]
    for g in groups:
        for p in range(P):
            g[p].fill_synthetic(11, p)
    p_ = np.arange(P, dtype=np.float64)
    scales = Bucket.from_numpy(((1.0 + np.mod(0.37 * p_, 1.0)) / 3.0 * 2.0 ** (np.mod(p_, 5) - 2)).astype(np.float32))
    t = Bucket.from_numpy(np.array([0.7123], np.float32))
    amax = Bucket.from_numpy(np.zeros(1, np.float32))
    fmi_amd.sync()
    S = args.sets
    launches = {
        "unscaled": lambda k: fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, groups[k % S][P], groups[k % S][:P], accumulate_f32=True),
        "scaled": lambda k: fmi_amd.reduce_tree_scaled(Alg.ALLREDUCE, groups[k % S][P], groups[k % S][:P], scales, t),
        "scaled_amax": lambda k: fmi_amd.reduce_tree_scaled(Alg.ALLREDUCE, groups[k % S][P], groups[k % S][:P], scales, t, amax),
        "scaled_f32": lambda k: fmi_amd.reduce_tree_scaled(Alg.ALLREDUCE, wide[k % S], groups[k % S][:P], scales, t),
    }
    algo = {r: P * n + n * (4 if r == "scaled_f32" else 1) for r in ROWS}
    rates = {r: [] for r in ROWS}
    for _ in range(PASSES):
        for r in ROWS:
            ms = timed(launches[r], args.iters, S)
            rates[r].append(algo[r] / (ms * 1e-3))
    yard = rates[ROWS[0]]
    spread = lambda xs: round((max(xs) - min(xs)) / statistics.median(xs), 4)  # noqa: E731
    lines = []
    for r in ROWS:
        ratios = [a / b for a, b in zip(rates[r], yard)]
        lines.append({"tool": "tools/fp8_scaled_bench.py", "label": args.label, "inflight_kib": fmi_amd.tune_get(fmi_amd.Tune.FUSED_INFLIGHT_KIB), "kernel": f"tree{P} {args.kind} {r}",
                      "algorithmic_bytes": algo[r], "iters_per_pass": args.iters, "passes": PASSES, "rotating_sets": S,
                      "GB_s_per_pass": [round(x / 1e9, 1) for x in rates[r]], "GB_s": round(statistics.median(rates[r]) / 1e9, 1),
                      "fraction_of_8TBs_per_pass": [round(x / PEAK, 4) for x in rates[r]],
                      "fraction_of_8TBs": round(statistics.median(rates[r]) / PEAK, 4), "spread": spread(rates[r]),
                      "yardstick": f"tree{P} {args.kind} {ROWS[0]}, same passes",
                      "ratio_to_unscaled_per_pass": [round(x, 4) for x in ratios],
                      "ratio_to_unscaled": round(statistics.median(ratios), 4), "unscaled_spread": spread(yard),
                      "timing": "two HIP events around back-to-back launches on the library stream"})
    emit(lines, args.out)
    for b in [b for g in groups for b in g] + wide + [scales, t, amax]:
        b.free()
    fmi_amd.sync()


if __name__ == "__main__":
    main()
