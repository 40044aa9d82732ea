"""The fused MX kernel (fmi_dev_reduce_tree_mx) beside the per-tensor scaled kernel and its own fallback, on one GPU,
timed with events, by the protocol of tools/fp8_scaled_bench.py:

  scaled            reduce_tree_scaled, out = the inputs' dtype, amax = NULL (the yardstick: its code is not the MX call's)
  mx                reduce_tree_mx SUM, out = the inputs' dtype with scale bytes: the fused kernel
  mx_f32            the same with an F32 output and no output scales
  mx_fallback       reduce_tree_mx on element buckets one byte off 16-B alignment: dequantize x P, the f32 program,
                    quantize (the path of P = 1, P > 16 and unaligned buckets)

P = 8 peers of 256 MiB of elements each (8 MiB of scale bytes per peer), the element buckets (and the 8-bit output) of a
set carved as one group (fmi_dev_alloc_group); three rotating sets, so that no bucket returns within 256 MB of the
Infinity Cache; the kernels interleaved in one process, three passes. One JSON line per kernel: element rate and bytes/s
per pass and their median, the fraction of 8 TB/s (algorithmic bytes, scale bytes counted: P * (n + n / 32) in,
n + n / 32 or 4 n out), the ratio of the ELEMENT rate to the yardstick's of the same pass, and the yardstick's own
spread over the passes.

    python3 tools/mx_bench.py [--kind e4m3] [--label NAME] [--out profiles/mx_bench.jsonl]

--kind e2m1: the fused MXFP4 kernel (FMI_F4E2M1 elements, two to a byte) instead, with the unchanged fused MXFP8 E4M3
kernel as the yardstick, in the same passes and at the same ELEMENT count (so the MXFP4 buckets are half the bytes):

  mx                reduce_tree_mx on E4M3 buckets, out = E4M3 with scale bytes (the yardstick)
  mxfp4             reduce_tree_mx on F4E2M1 buckets, out = F4E2M1 with scale bytes: the fused kernel
  mx_f32            the yardstick's kernel with an F32 output: what mxfp4_f32 stands beside (both store 4 n bytes)
  mxfp4_f32         the fused MXFP4 kernel with an F32 output
  mxfp4_fallback    the same buckets one byte off 16-B alignment

Bytes with the scale bytes counted: inputs P * (n / 2 + n / 32), output n / 2 + n / 32 or 4 n.

    python3 tools/mx_bench.py --kind e2m1 [--label NAME] [--out profiles/mxfp4_bench.jsonl]

--kind e2m3 / --kind e3m2: the fused MXFP6 kernel (FMI_F6E2M3 / FMI_F6E3M2 elements, four to three bytes) by the same
protocol, with the unchanged fused MXFP8 E4M3 kernel as the yardstick, in the same passes and at the same ELEMENT count:

  mx                reduce_tree_mx on E4M3 buckets, out = E4M3 with scale bytes (the yardstick)
  mxfp6             reduce_tree_mx on FP6 buckets, out = FP6 with scale bytes: the fused kernel
  mx_f32            the yardstick's kernel with an F32 output: what mxfp6_f32 stands beside (both store 4 n bytes)
  mxfp6_f32         the fused MXFP6 kernel with an F32 output
  mxfp6_sr          the fused MXFP6 kernel with stochastic rounding
  mxfp6_fallback    the same buckets three bytes off 16-B alignment

Bytes with the scale bytes counted: inputs P * (3 n / 4 + n / 32), output 3 n / 4 + n / 32 or 4 n.

    python3 tools/mx_bench.py --kind e2m3 [--label NAME] [--out profiles/mxfp6_bench.jsonl]

--sr: the stochastic-rounding kernels (fmi_dev_reduce_tree_mx_sr) beside the round-to-nearest ones, whose code is
unchanged, in the same passes at the same element count:

  mx                          reduce_tree_mx on E4M3 buckets, out = E4M3 (yardstick of mx_sr)
  mxfp4                       reduce_tree_mx on F4E2M1 buckets, out = F4E2M1 (yardstick of mxfp4_sr)
  mx_sr, mxfp4_sr             the same calls with a seed: the fused stochastic-rounding kernels
  mx_f32_then_quantize_sr,    the fused kernel of the same element type with an F32 output, then mx_quantize with the
  mxfp4_f32_then_quantize_sr  seed: the only way to stochastic rounding without the fused variant (8 n more bytes per call)

Each row carries its element rate per pass and the ratio to its yardstick; the two fused rows also carry the ratio to the
two-kernel composition of their own element type per pass and whether it exceeds 1 in every pass.

    python3 tools/mx_bench.py --sr [--label NAME] [--out profiles/mx_sr_bench.jsonl]
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

ROWS = ("scaled", "mx", "mx_f32", "mx_fallback")  # the first is the yardstick
PEAK = 8e12


FP4_ROWS = ("mx", "mxfp4", "mx_f32", "mxfp4_f32", "mxfp4_fallback")  # the first is the yardstick


def main_e2m1(args):
    """n ELEMENTS per peer: E4M3 buckets of n bytes for the yardstick, F4E2M1 buckets of n / 2 bytes."""
    P, n, S = args.peers, args.mib * MIB, args.sets
    nb = fmi_amd.mx_blocks(n)
    rows = [r for r in FP4_ROWS if r == FP4_ROWS[0] or r in args.rows.split(",")]
    g8 = [Bucket.group(P + 1, n, DType.F8E4M3) for _ in range(S)]
    # 16 spare bytes (32 elements) per bucket: the fallback's buckets are the same allocations one byte in
    g4 = [Bucket.group(P + 1, n + 32, DType.F4E2M1) for _ in range(S)]
    aligned = [[b.view(0, n) for b in g] for g in g4]
    shifted = [[b.view(2, n) for b in g] for g in g4]
    wide = [Bucket(n, np.float32) for _ in range(S)]
    rng = np.random.default_rng(3)
    packed = rng.integers(0, 256, n // 2 + 16, dtype=np.uint8)  # every nibble; the buckets differ by a rotation of the codes
    scale_sets = []
    for k in range(S):
        for p in range(P):
            g8[k][p].fill_synthetic(11, p)
            g4[k][p].upload(packed ^ np.uint8(17 * (k * P + p) & 0xFF))
        scale_sets.append([Bucket(nb, DType.F8E8M0) for _ in range(P + 1)])
        for b in scale_sets[-1][:P]:
            b.upload(rng.integers(120, 135, nb).astype(np.uint8))
    fmi_amd.sync()
    tree = lambda out, osc, ins, k: fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, out, osc, ins, scale_sets[k % S][:P])  # noqa: E731
    launches = {
        "mx": lambda k: tree(g8[k % S][P], scale_sets[k % S][P], g8[k % S][:P], k),
        "mxfp4": lambda k: tree(aligned[k % S][P], scale_sets[k % S][P], aligned[k % S][:P], k),
        "mx_f32": lambda k: tree(wide[k % S], None, g8[k % S][:P], k),
        "mxfp4_f32": lambda k: tree(wide[k % S], None, aligned[k % S][:P], k),
        "mxfp4_fallback": lambda k: tree(shifted[k % S][P], scale_sets[k % S][P], shifted[k % S][:P], k),
    }
    algo = {"mx": P * (n + nb) + n + nb, "mx_f32": P * (n + nb) + 4 * n, "mxfp4": P * (n // 2 + nb) + n // 2 + nb, "mxfp4_f32": P * (n // 2 + nb) + 4 * n,
            "mxfp4_fallback": P * (n // 2 + nb) + n // 2 + nb}
    iters = {r: args.fallback_iters if r == "mxfp4_fallback" else args.iters for r in FP4_ROWS}
    ms = {r: [] for r in rows}
    for _ in range(PASSES):
        for r in rows:
            ms[r].append(timed(launches[r], iters[r], S))
    spread = lambda xs: round((max(xs) - min(xs)) / statistics.median(xs), 4)  # noqa: E731
    elem = {r: [n / (m * 1e-3) for m in ms[r]] for r in rows}
    lines = []
    for r in rows:
        byte_rate = [algo[r] / (m * 1e-3) for m in ms[r]]
        ratios = [a / b for a, b in zip(elem[r], elem[FP4_ROWS[0]])]
        lines.append({"tool": "tools/mx_bench.py --kind e2m1", "label": args.label, "inflight_kib": fmi_amd.tune_get(fmi_amd.Tune.FUSED_INFLIGHT_KIB),
                      "kernel": f"tree{P} {'e4m3' if r in ('mx', 'mx_f32') else 'e2m1'} {r}", "elements_per_peer": n, "algorithmic_bytes": algo[r],
                      "bytes_per_element": round(algo[r] / n, 4),
                      "iters_per_pass": iters[r], "passes": PASSES, "rotating_sets": S, "ms_per_pass": [round(m, 4) for m in ms[r]],
                      "Gelem_s_per_pass": [round(x / 1e9, 2) for x in elem[r]], "Gelem_s": round(statistics.median(elem[r]) / 1e9, 2),
                      "GB_s_per_pass": [round(x / 1e9, 1) for x in byte_rate], "GB_s": round(statistics.median(byte_rate) / 1e9, 1),
                      "fraction_of_8TBs": round(statistics.median(byte_rate) / PEAK, 4), "spread": spread(byte_rate),
                      "yardstick": f"tree{P} e4m3 mx (the fused MXFP8 kernel), same passes, same element count, element rate",
                      "element_rate_ratio_to_mxfp8_per_pass": [round(x, 4) for x in ratios],
                      "element_rate_ratio_to_mxfp8": round(statistics.median(ratios), 4), "mxfp8_spread": spread(elem[FP4_ROWS[0]]),
                      "timing": "two HIP events around back-to-back launches on the library stream"})
    emit(lines, args.out)
    for b in [b for g in g8 + g4 for b in g] + wide + [b for s in scale_sets for b in s]:
        b.free()
    fmi_amd.sync()


FP6_ROWS = ("mx", "mxfp6", "mx_f32", "mxfp6_f32", "mxfp6_sr", "mxfp6_fallback")  # the first is the yardstick


def main_fp6(args):
    """n ELEMENTS per peer: E4M3 buckets of n bytes for the yardstick, FP6 buckets of 3 n / 4 bytes."""
    P, n, S = args.peers, args.mib * MIB, args.sets
    dt = DType.F6E2M3 if args.kind == "e2m3" else DType.F6E3M2
    nb = fmi_amd.mx_blocks(n)
    rows = [r for r in FP6_ROWS if r == FP6_ROWS[0] or r in args.rows.split(",")]
    g8 = [Bucket.group(P + 1, n, DType.F8E4M3) for _ in range(S)]
    # 48 spare bytes (64 elements) per bucket: the fallback's buckets are the same allocations three bytes in
    g6 = [Bucket.group(P + 1, n + 64, dt) for _ in range(S)]
    aligned = [[b.view(0, n) for b in g] for g in g6]
    shifted = [[b.view(4, n) for b in g] for g in g6]
    wide = [Bucket(n, np.float32) for _ in range(S)]
    seed = Bucket.from_numpy(np.array([0x0123456789ABCDEF], np.uint64))
    rng = np.random.default_rng(3)
    packed = rng.integers(0, 256, n // 4 * 3 + 48, dtype=np.uint8)  # every code; the buckets differ by a flip of code bits
    scale_sets = []
    for k in range(S):
        for p in range(P):
            g8[k][p].fill_synthetic(11, p)
            g6[k][p].upload(packed ^ np.uint8(17 * (k * P + p) & 0xFF))
        scale_sets.append([Bucket(nb, DType.F8E8M0) for _ in range(P + 1)])
        for b in scale_sets[-1][:P]:
            b.upload(rng.integers(120, 135, nb).astype(np.uint8))
    fmi_amd.sync()
    tree = lambda out, osc, ins, k, **kw: fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, out, osc, ins, scale_sets[k % S][:P], **kw)  # noqa: E731
    launches = {
        "mx": lambda k: tree(g8[k % S][P], scale_sets[k % S][P], g8[k % S][:P], k),
        "mxfp6": lambda k: tree(aligned[k % S][P], scale_sets[k % S][P], aligned[k % S][:P], k),
        "mx_f32": lambda k: tree(wide[k % S], None, g8[k % S][:P], k),
        "mxfp6_f32": lambda k: tree(wide[k % S], None, aligned[k % S][:P], k),
        "mxfp6_sr": lambda k: tree(aligned[k % S][P], scale_sets[k % S][P], aligned[k % S][:P], k, seed=seed, first=0),
        "mxfp6_fallback": lambda k: tree(shifted[k % S][P], scale_sets[k % S][P], shifted[k % S][:P], k),
    }
    e6 = n // 4 * 3
    algo = {"mx": P * (n + nb) + n + nb, "mx_f32": P * (n + nb) + 4 * n, "mxfp6": P * (e6 + nb) + e6 + nb, "mxfp6_f32": P * (e6 + nb) + 4 * n,
            "mxfp6_sr": P * (e6 + nb) + e6 + nb, "mxfp6_fallback": P * (e6 + nb) + e6 + nb}
    iters = {r: args.fallback_iters if r == "mxfp6_fallback" else args.iters for r in FP6_ROWS}
    ms = {r: [] for r in rows}
    for _ in range(PASSES):
        for r in rows:
            ms[r].append(timed(launches[r], iters[r], S))
    spread = lambda xs: round((max(xs) - min(xs)) / statistics.median(xs), 4)  # noqa: E731
    elem = {r: [n / (m * 1e-3) for m in ms[r]] for r in rows}
    lines = []
    for r in rows:
        byte_rate = [algo[r] / (m * 1e-3) for m in ms[r]]
        ratios = [a / b for a, b in zip(elem[r], elem[FP6_ROWS[0]])]
        lines.append({"tool": f"tools/mx_bench.py --kind {args.kind}", "label": args.label, "inflight_kib": fmi_amd.tune_get(fmi_amd.Tune.FUSED_INFLIGHT_KIB),
                      "kernel": f"tree{P} {'e4m3' if r in ('mx', 'mx_f32') else args.kind} {r}", "elements_per_peer": n, "algorithmic_bytes": algo[r],
                      "bytes_per_element": round(algo[r] / n, 4),
                      "iters_per_pass": iters[r], "passes": PASSES, "rotating_sets": S, "ms_per_pass": [round(m, 4) for m in ms[r]],
                      "ms_per_call": round(statistics.median(ms[r]), 4),
                      "Gelem_s_per_pass": [round(x / 1e9, 2) for x in elem[r]], "Gelem_s": round(statistics.median(elem[r]) / 1e9, 2),
                      "GB_s_per_pass": [round(x / 1e9, 1) for x in byte_rate], "GB_s": round(statistics.median(byte_rate) / 1e9, 1),
                      "fraction_of_8TBs": round(statistics.median(byte_rate) / PEAK, 4), "spread": spread(byte_rate),
                      "yardstick": f"tree{P} e4m3 mx (the fused MXFP8 kernel), same passes, same element count, element rate",
                      "element_rate_ratio_to_mxfp8_per_pass": [round(x, 4) for x in ratios],
                      "element_rate_ratio_to_mxfp8": round(statistics.median(ratios), 4),
                      "at_least_mxfp8_in_every_pass": all(x >= 1.0 for x in ratios), "mxfp8_spread": spread(elem[FP6_ROWS[0]]),
                      "timing": "two HIP events around back-to-back launches on the library stream"})
    emit(lines, args.out)
    for b in [b for g in g8 + g6 for b in g] + wide + [b for s in scale_sets for b in s] + [seed]:
        b.free()
    fmi_amd.sync()


SR_ROWS = ("mx", "mxfp4", "mx_sr", "mxfp4_sr", "mx_f32_then_quantize_sr", "mxfp4_f32_then_quantize_sr")
SR_YARDSTICK = {"mx": "mx", "mxfp4": "mxfp4", "mx_sr": "mx", "mxfp4_sr": "mxfp4", "mx_f32_then_quantize_sr": "mx",
                "mxfp4_f32_then_quantize_sr": "mxfp4"}
SR_COMPOSITION = {"mx_sr": "mx_f32_then_quantize_sr", "mxfp4_sr": "mxfp4_f32_then_quantize_sr"}


def main_sr(args):
    """n ELEMENTS per peer, as main_e2m1: E4M3 buckets of n bytes, F4E2M1 buckets of n / 2 bytes."""
    P, n, S = args.peers, args.mib * MIB, args.sets
    nb = fmi_amd.mx_blocks(n)
    g8 = [Bucket.group(P + 1, n, DType.F8E4M3) for _ in range(S)]
    g4 = [Bucket.group(P + 1, n, DType.F4E2M1) for _ in range(S)]
    wide = [Bucket(n, np.float32) for _ in range(S)]
    seed = Bucket.from_numpy(np.array([0x0123456789ABCDEF], np.uint64))
    rng = np.random.default_rng(3)
    packed = rng.integers(0, 256, n // 2, dtype=np.uint8)
    scale_sets = []
    for k in range(S):
        for p in range(P):
            g8[k][p].fill_synthetic(11, p)
            g4[k][p].upload(packed ^ np.uint8(17 * (k * P + p) & 0xFF))
        scale_sets.append([Bucket(nb, DType.F8E8M0) for _ in range(P + 1)])
        for b in scale_sets[-1][:P]:
            b.upload(rng.integers(120, 135, nb).astype(np.uint8))
    fmi_amd.sync()

    def tree(g, k, out=None, **kw):
        s = scale_sets[k % S]
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, g[k % S][P] if out is None else out, s[P] if out is None else None, g[k % S][:P], s[:P], **kw)

    def composition(g):
        def launch(k):
            tree(g, k, out=wide[k % S])
            fmi_amd.mx_quantize(g[k % S][P], scale_sets[k % S][P], wide[k % S], seed=seed, first=0)
        return launch

    launches = {
        "mx": lambda k: tree(g8, k),
        "mxfp4": lambda k: tree(g4, k),
        "mx_sr": lambda k: tree(g8, k, seed=seed, first=0),
        "mxfp4_sr": lambda k: tree(g4, k, seed=seed, first=0),
        "mx_f32_then_quantize_sr": composition(g8),
        "mxfp4_f32_then_quantize_sr": composition(g4),
    }
    in8, in4, out8, out4 = P * (n + nb), P * (n // 2 + nb), n + nb, n // 2 + nb
    algo = {"mx": in8 + out8, "mx_sr": in8 + out8, "mxfp4": in4 + out4, "mxfp4_sr": in4 + out4,
            "mx_f32_then_quantize_sr": in8 + 8 * n + out8, "mxfp4_f32_then_quantize_sr": in4 + 8 * n + out4}
    ms = {r: [] for r in SR_ROWS}
    for _ in range(PASSES):
        for r in SR_ROWS:
            ms[r].append(timed(launches[r], args.iters, S))
    spread = lambda xs: round((max(xs) - min(xs)) / statistics.median(xs), 4)  # noqa: E731
    elem = {r: [n / (m * 1e-3) for m in ms[r]] for r in SR_ROWS}
    lines = []
    for r in SR_ROWS:
        byte_rate = [algo[r] / (m * 1e-3) for m in ms[r]]
        ratios = [a / b for a, b in zip(elem[r], elem[SR_YARDSTICK[r]])]
        line = {"tool": "tools/mx_bench.py --sr", "label": args.label, "inflight_kib": fmi_amd.tune_get(fmi_amd.Tune.FUSED_INFLIGHT_KIB),
                "kernel": f"tree{P} {'e4m3' if SR_YARDSTICK[r] == 'mx' else 'e2m1'} {r}", "elements_per_peer": n, "algorithmic_bytes": algo[r],
                "bytes_per_element": round(algo[r] / n, 4), "iters_per_pass": args.iters, "passes": PASSES, "rotating_sets": S,
                "ms_per_pass": [round(m, 4) for m in ms[r]], "Gelem_s_per_pass": [round(x / 1e9, 2) for x in elem[r]],
                "Gelem_s": round(statistics.median(elem[r]) / 1e9, 2), "GB_s_per_pass": [round(x / 1e9, 1) for x in byte_rate],
                "GB_s": round(statistics.median(byte_rate) / 1e9, 1), "fraction_of_8TBs": round(statistics.median(byte_rate) / PEAK, 4),
                "spread": spread(byte_rate), "yardstick": f"tree{P} {SR_YARDSTICK[r]} (round to nearest, code unchanged), same passes, element rate",
                "element_rate_ratio_to_rne_per_pass": [round(x, 4) for x in ratios], "element_rate_ratio_to_rne": round(statistics.median(ratios), 4),
                "timing": "two HIP events around back-to-back launches on the library stream"}
        if r in SR_COMPOSITION:
            over = [a / b for a, b in zip(elem[r], elem[SR_COMPOSITION[r]])]
            line["composition"] = SR_COMPOSITION[r]
            line["element_rate_ratio_to_composition_per_pass"] = [round(x, 4) for x in over]
            line["exceeds_composition_in_every_pass"] = all(x > 1.0 for x in over)
        lines.append(line)
    emit(lines, args.out)
    for b in [b for g in g8 + g4 for b in g] + wide + [b for s in scale_sets for b in s] + [seed]:
        b.free()
    fmi_amd.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="e4m3", choices=("e4m3", "e5m2", "e2m1", "e2m3", "e3m2"))
    ap.add_argument("--mib", type=int, default=256, help="element bytes per input bucket")
    ap.add_argument("--peers", type=int, default=8)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--iters", type=int, default=24, help="timed launches per fused kernel and pass")
    ap.add_argument("--fallback-iters", type=int, default=3, help="timed calls of the fallback per pass (about ten times the bytes)")
    ap.add_argument("--rows", default=",".join(ROWS), help="which rows to run; the yardstick always runs")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--sr", action="store_true", help="the stochastic-rounding rows beside the round-to-nearest kernels")
    args = ap.parse_args()
    fmi_amd.init(0)
    if args.sr:
        return main_sr(args)
    if args.kind == "e2m1":
        if args.rows == ",".join(ROWS):
            args.rows = ",".join(FP4_ROWS)
        return main_e2m1(args)
    if args.kind in ("e2m3", "e3m2"):
        if args.rows == ",".join(ROWS):
            args.rows = ",".join(FP6_ROWS)
        return main_fp6(args)
    dt = DType.F8E4M3 if args.kind == "e4m3" else DType.F8E5M2
    P, n, S = args.peers, args.mib * MIB, args.sets
    nb = fmi_amd.mx_blocks(n)
    rows = [r for r in ROWS if r == ROWS[0] or r in args.rows.split(",")]
    # 16 spare bytes per bucket: the fallback's inputs are the same allocations one byte in
    groups = [Bucket.group(P + 1, n + 16, dt) for _ in range(S)]
    aligned = [[b.view(0, n) for b in g] for g in groups]
    shifted = [[b.view(1, n) for b in g] for g in groups]
    wide = [Bucket(n, np.float32) for _ in range(S)]
    rng = np.random.default_rng(3)
    scale_sets = []
    for g in aligned:
        for p in range(P):
            g[p].fill_synthetic(11, p)
        scale_sets.append([Bucket(nb, DType.F8E8M0) for _ in range(P + 1)])
        for b in scale_sets[-1][:P]:
            b.upload(rng.integers(120, 135, nb).astype(np.uint8))
    p_ = np.arange(P, dtype=np.float64)
    scales = Bucket.from_numpy(((1.0 + np.mod(0.37 * p_, 1.0)) / 3.0 * 2.0 ** (np.mod(p_, 5) - 2)).astype(np.float32))
    t = Bucket.from_numpy(np.array([0.7123], np.float32))
    fmi_amd.sync()
    launches = {
        "scaled": lambda k: fmi_amd.reduce_tree_scaled(Alg.ALLREDUCE, aligned[k % S][P], aligned[k % S][:P], scales, t),
        "mx": lambda k: fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, aligned[k % S][P], scale_sets[k % S][P], aligned[k % S][:P], scale_sets[k % S][:P]),
        "mx_f32": lambda k: fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, wide[k % S], None, aligned[k % S][:P], scale_sets[k % S][:P]),
        "mx_fallback": lambda k: fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, shifted[k % S][P], scale_sets[k % S][P], shifted[k % S][:P], scale_sets[k % S][:P]),
    }
    algo = {"scaled": P * n + n, "mx": P * (n + nb) + n + nb, "mx_f32": P * (n + nb) + 4 * n, "mx_fallback": P * (n + nb) + n + nb}
    iters = {r: args.fallback_iters if r == "mx_fallback" else args.iters for r in ROWS}
    ms = {r: [] for r in rows}
    for _ in range(PASSES):
        for r in rows:
            ms[r].append(timed(launches[r], iters[r], S))
    spread = lambda xs: round((max(xs) - min(xs)) / statistics.median(xs), 4)  # noqa: E731
    elem = {r: [n / (m * 1e-3) for m in ms[r]] for r in rows}
    lines = []
    for r in rows:
        byte_rate = [algo[r] / (m * 1e-3) for m in ms[r]]
        ratios = [a / b for a, b in zip(elem[r], elem[ROWS[0]])]
        lines.append({"tool": "tools/mx_bench.py", "label": args.label, "inflight_kib": fmi_amd.tune_get(fmi_amd.Tune.FUSED_INFLIGHT_KIB),
                      "kernel": f"tree{P} {args.kind} {r}", "elements_per_peer": n, "algorithmic_bytes": algo[r],
                      "iters_per_pass": iters[r], "passes": PASSES, "rotating_sets": S, "ms_per_pass": [round(m, 4) for m in ms[r]],
                      "Gelem_s_per_pass": [round(x / 1e9, 2) for x in elem[r]], "Gelem_s": round(statistics.median(elem[r]) / 1e9, 2),
                      "GB_s_per_pass": [round(x / 1e9, 1) for x in byte_rate], "GB_s": round(statistics.median(byte_rate) / 1e9, 1),
                      "fraction_of_8TBs": round(statistics.median(byte_rate) / PEAK, 4), "spread": spread(byte_rate),
                      "yardstick": f"tree{P} {args.kind} {ROWS[0]}, same passes, element rate",
                      "element_rate_ratio_to_scaled_per_pass": [round(x, 4) for x in ratios],
                      "element_rate_ratio_to_scaled": round(statistics.median(ratios), 4), "scaled_spread": spread(elem[ROWS[0]]),
                      "timing": "two HIP events around back-to-back launches on the library stream"})
    emit(lines, args.out)
    for b in [b for g in groups for b in g] + wide + [b for s in scale_sets for b in s] + [scales, t]:
        b.free()
    fmi_amd.sync()


if __name__ == "__main__":
    main()
