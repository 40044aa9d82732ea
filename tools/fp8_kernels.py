"""The 8-bit float kernels (FMI_F8E4M3, FMI_F8E5M2) beside the bf16 kernel of EQUAL BYTES, on one GPU, timed with events,
by the protocol of tools/half_kernels.py:

  pair       fmi_dev_reduce_pair SUM at 256 MiB per bucket: bf16 (the yardstick), e4m3, e5m2
             (3 x 256 MiB algorithmic bytes per launch; 16 rotating sets of two buckets)
  tree8      the fused 8-way ALLREDUCE with FMI_ACC_F32 over a carved group (fmi_dev_alloc_group, 8 inputs + the
             output) at 256 MiB per bucket: bf16 acc32 (the yardstick), e4m3 acc32, e5m2 acc32
             (9 x 256 MiB per launch; 3 rotating groups)
  tree16     the same over 16 peers (17 x 256 MiB per launch; 2 rotating groups)
  convert    fmi_dev_convert of 1 GiB of f32: to bf16 (the yardstick: 1.5 GiB moved), to e4m3 and e5m2 (1.25 GiB moved)
             (3 rotating sets)

Every set is far larger than what the 256 MB Infinity Cache could hold back for its next use. The kernels of a family
are interleaved, three passes over all of them, so drift of the device hits every kernel alike. One JSON line per
kernel: bytes/s per pass and their median, the ratio to the bf16 yardstick of the same family in the same pass, and
the spread of that yardstick against itself over the three passes ((max - min) / median): an 8-bit row more than that
spread below its yardstick is a finding (never the 8-bit kernel against itself).

    python3 tools/fp8_kernels.py [--only pair,tree8,tree16,convert] [--label NAME] [--out profiles/fp8_kernels.jsonl]
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

DTYPES = {"bf16": (DType.BF16, 2), "e4m3": (DType.F8E4M3, 1), "e5m2": (DType.F8E5M2, 1)}
ROWS = ("bf16", "e4m3", "e5m2")  # the first is the yardstick


def free_all(buckets):
    for b in buckets:
        b.free()
    fmi_amd.sync()


def family(args, fam, launches, algo, warm, sets, what):
    """launches: {row: launch(k)}; algo: {row: algorithmic bytes per launch}."""
    rates = {r: [] for r in ROWS}
    for _ in range(PASSES):
        for r in ROWS:
            ms = timed(launches[r], args.iters, warm)
            rates[r].append(algo[r] / (ms * 1e-3))
    yard = rates[ROWS[0]]
    spread = lambda xs: round((max(xs) - min(xs)) / statistics.median(xs), 4)  # noqa: E731
    lines = []
    for r in ROWS:
        ratios = [a / b for a, b in zip(rates[r], yard)]
        lines.append({"tool": "tools/fp8_kernels.py", "label": args.label, "kernel": f"{fam} {r} {what}",
                      "algorithmic_bytes": algo[r], "iters_per_pass": args.iters, "passes": PASSES, "rotating_sets": sets,
                      "GB_s_per_pass": [round(x / 1e9, 1) for x in rates[r]],
                      "bytes_per_s": round(statistics.median(rates[r])), "GB_s": round(statistics.median(rates[r]) / 1e9, 1),
                      "spread": spread(rates[r]), "yardstick": f"{fam} {ROWS[0]} {what}, same passes",
                      "ratio_to_bf16_per_pass": [round(x, 4) for x in ratios],
                      "ratio_to_bf16": round(statistics.median(ratios), 4), "bf16_spread": spread(yard),
                      "timing": "two HIP events around back-to-back launches on the library stream"})
    emit(lines, args.out)


def pair(args):
    nbytes = args.mib * MIB
    sets = {r: [tuple(Bucket(nbytes // DTYPES[r][1], DTYPES[r][0]).fill_synthetic(42 + s, j) for j in range(2))
                for s in range(args.pair_sets)] for r in ROWS}
    fmi_amd.sync()
    launches = {r: (lambda k, s=sets[r]: fmi_amd.reduce_pair(Op.SUM, *s[k % len(s)])) for r in ROWS}
    family(args, "pair", launches, {r: 3 * nbytes for r in ROWS}, args.pair_sets, args.pair_sets, "sum")
    free_all([b for ss in sets.values() for s in ss for b in s])


def tree(args, P, nsets):
    nbytes = args.mib * MIB
    groups = {}
    for r in ROWS:
        dt, esz = DTYPES[r]
        groups[r] = [Bucket.group(P + 1, nbytes // esz, dt) for _ in range(nsets)]
        for g in groups[r]:
            for p in range(P):
                g[p].fill_synthetic(11, p)
    fmi_amd.sync()
    launches = {r: (lambda k, gs=groups[r]: fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, gs[k % len(gs)][P], gs[k % len(gs)][:P],
                                                                 accumulate_f32=True)) for r in ROWS}
    family(args, f"tree{P}", launches, {r: (P + 1) * nbytes for r in ROWS}, nsets, nsets, "acc32 sum")
    free_all([b for gs in groups.values() for g in gs for b in g])


def convert(args):
    n = args.convert_mib * MIB // 4
    nsets = 3
    srcs = [Bucket(n, np.float32).fill_synthetic(7 + s, 0) for s in range(nsets)]
    dsts = {r: [Bucket(n, DTYPES[r][0]) for _ in range(nsets)] for r in ROWS}
    fmi_amd.sync()
    launches = {r: (lambda k, d=dsts[r]: fmi_amd.convert(d[k % nsets], srcs[k % nsets])) for r in ROWS}
    family(args, "convert", launches, {r: n * (4 + DTYPES[r][1]) for r in ROWS}, nsets, nsets, f"from {args.convert_mib} MiB of f32")
    free_all(srcs + [b for d in dsts.values() for b in d])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256, help="bytes per bucket (pair, tree)")
    ap.add_argument("--convert-mib", type=int, default=1024, help="bytes of f32 per conversion")
    ap.add_argument("--iters", type=int, default=32, help="timed launches per kernel and pass")
    ap.add_argument("--pair-sets", type=int, default=16)
    ap.add_argument("--only", default="pair,tree8,tree16,convert")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    fmi_amd.init(0)
    for fam in args.only.split(","):
        if fam == "pair":
            pair(args)
        elif fam == "tree8":
            tree(args, 8, 3)
        elif fam == "tree16":
            tree(args, 16, 2)
        elif fam == "convert":
            convert(args)
        else:
            sys.exit(f"unknown family {fam}")


if __name__ == "__main__":
    main()
