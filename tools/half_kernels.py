"""The 16-bit float kernels against the f32 kernels of equal bytes, on one GPU, timed with events:

  pair     fmi_dev_reduce_pair at 256 MiB per bucket: f32 sum, f16 sum, bf16 sum, bf16 max
           (3 x 256 MiB algorithmic bytes per launch; 16 rotating sets of two buckets, as bench.py's C2)
  tree8    the fused 8-way allreduce (fmi_dev_reduce_tree, ALLREDUCE) over a carved group (fmi_dev_alloc_group,
           8 inputs + the output) at 256 MiB per bucket: f32 sum, bf16 sum
           (9 x 256 MiB per launch; 3 rotating groups, as bench.py's c4_one_gpu)

With --forms, the fused forms beyond the 8-way allreduce instead, each family allocated, measured and freed in turn:

  reduce_ltr8   REDUCE_LTR over 8 peers: f32 sum, bf16 sum              (9 x 256 MiB per launch; 3 groups)
  scan_ltr8     SCAN_LTR over 8 peers: f32 sum, bf16 sum                (16 x 256 MiB; 3 groups)
  reduce32      REDUCE over 32 peers: f32 sum, bf16 sum, f32 max, f16 max (33 x 256 MiB; 2 groups)
  allreduce24   ALLREDUCE over 24 peers, rank 17 (float max: the rank-selecting kernel): f32 max, bf16 max
                                                                        (25 x 256 MiB; 2 groups)
  scan32        SCAN over 32 peers: f32 sum, bf16 sum                   (64 x 256 MiB; 2 groups)
  allreduce13   (only with --only) ALLREDUCE over 13 peers, rank 5: f32 max, bf16 max (14 x 256 MiB; 3 groups)

With --acc32, the f32-accumulating kernels (FMI_ACC_F32, accumulate_f32=True) beside the plain 16-bit kernel of the same
shape (same bytes) and the f32 kernel of equal bytes, sum, for bf16 and f16:

  allreduce8    ALLREDUCE over 8 peers   (9 x 256 MiB per launch; 3 groups)
  scan8         SCAN over 8 peers        (16 x 256 MiB; 3 groups)
  reduce_ltr16  REDUCE_LTR over 16 peers (17 x 256 MiB; 2 groups)
  scan16        SCAN over 16 peers       (32 x 256 MiB; 2 groups)

Each line carries its own spread over the three passes, its ratio to the plain 16-bit kernel and to f32 per pass.

With --avg, the mean (FMI_OP_AVG) beside SUM of the same shape run by ANOTHER build of the library (--yardstick-lib,
e.g. the parent commit's libfmi_dev.so), both loaded into this process and interleaved in the same passes over the
same buckets:

  allreduce8    ALLREDUCE over 8 peers: f32, bf16, bf16 acc32    (9 x 256 MiB per launch; 3 groups)  one fused kernel
  allreduce16   ALLREDUCE over 16 peers: f32, bf16, bf16 acc32   (17 x 256 MiB; 2 groups)            one fused kernel
  allreduce17   ALLREDUCE over 17 peers: f32                     (18 x 256 MiB; 2 groups)  the SUM kernel, then the
                scale kernel: (P + 3) / (P + 1) of the SUM's traffic; reported beside that estimate, no bar

Each line carries the yardstick's rate per pass, the ratio per pass and the yardstick f32 SUM kernel's own spread
over the three passes: a fused row more than that spread below its yardstick is a finding.

The yardstick of a 16-bit kernel is the f32 kernel of the same family and op. The same rows run against any
library (FMI_DEV_LIB), e.g. one built from an earlier commit whose 16-bit programs ran as pairwise passes.

Every set is far larger than what the 256 MB Infinity Cache could hold back for its next use. The kernels are
interleaved, three passes over all of them, so drift of the device hits every kernel alike. One JSON line per
kernel: bytes/s per pass and their median, the ratio to the f32 kernel of the same family in the same pass, and
the spread of that f32 kernel against itself over the three passes ((max - min) / median): a 16-bit kernel more
than that spread below f32 is a finding.

    python3 tools/half_kernels.py [--out profiles/NAME.jsonl]
    python3 tools/half_kernels.py --acc32 [--only allreduce8,scan16] [--out profiles/NAME.jsonl]
    python3 tools/half_kernels.py --avg --yardstick-lib PATH/libfmi_dev.so [--out profiles/avg.jsonl]
    python3 tools/half_kernels.py --forms [--only reduce_ltr8,reduce32] [--label NAME] [--out profiles/NAME.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import fmi_amd  # noqa: E402
from fmi_amd import Alg, Bucket, DType, Event, Op  # noqa: E402

MIB = 1 << 20
PASSES = 3
DTYPES = {"f32": (np.float32, 4), "f16": (DType.F16, 2), "bf16": (DType.BF16, 2)}


def timed(launch, iters, warm):
    for k in range(warm):
        launch(k)
    e0, e1 = Event(), Event()
    e0.record()
    for k in range(warm, warm + iters):
        launch(k)
    e1.record()
    e1.sync()
    ms = e0.elapsed_ms(e1) / iters
    e0.destroy()
    e1.destroy()
    return ms


def emit(lines, path):
    out = open(path, "a") if path else None
    for line in lines:
        s = json.dumps(line)
        print(s, flush=True)
        if out:
            out.write(s + "\n")
    if out:
        out.close()


# family: (peers, buckets per group, rotating groups, launch(op, group), [(dtype, op, the f32 yardstick's name)])
def _reduce(alg, P, rank=0):
    return lambda op, g: fmi_amd.reduce_tree(op, alg, g[P], g[:P], rank=rank)


def _scan(alg, P):
    return lambda op, g: fmi_amd.scan_peers(op, alg, g[P:], g[:P])


FORMS = {
    "reduce_ltr8": (8, 9, 3, _reduce(Alg.REDUCE_LTR, 8), [("f32", "sum"), ("bf16", "sum")]),
    "scan_ltr8": (8, 16, 3, _scan(Alg.SCAN_LTR, 8), [("f32", "sum"), ("bf16", "sum")]),
    "reduce32": (32, 33, 2, _reduce(Alg.REDUCE, 32), [("f32", "sum"), ("bf16", "sum"), ("f32", "max"), ("f16", "max")]),
    "allreduce24": (24, 25, 2, _reduce(Alg.ALLREDUCE, 24, rank=17), [("f32", "max"), ("bf16", "max")]),
    "scan32": (32, 64, 2, _scan(Alg.SCAN, 32), [("f32", "sum"), ("bf16", "sum")]),
    # not in the default set (--only allreduce13): the rank-selecting kernel below 17 peers
    "allreduce13": (13, 14, 3, _reduce(Alg.ALLREDUCE, 13, rank=5), [("f32", "max"), ("bf16", "max")]),
}
OPS = {"sum": Op.SUM, "max": Op.MAX}


def forms(args):
    nbytes = args.mib * MIB
    for fam in (args.only.split(",") if args.only else [f for f in FORMS if f != "allreduce13"]):
        P, count, sets, launch, rows = FORMS[fam]
        groups = {}
        for name in {r[0] for r in rows}:
            dt, esz = DTYPES[name]
            groups[name] = [Bucket.group(count, nbytes // esz, dt) for _ in range(sets)]
            for g in groups[name]:
                for p in range(P):
                    g[p].fill_synthetic(11, p)
        fmi_amd.sync()
        rates = {r: [] for r in rows}
        for _ in range(PASSES):
            for name, op in rows:
                gs = groups[name]
                ms = timed(lambda k: launch(OPS[op], gs[k % len(gs)]), args.iters, sets)
                rates[(name, op)].append(count * nbytes / (ms * 1e-3))
        lines = []
        for name, op in rows:
            f32 = rates[("f32", op)]
            ratios = [r / y for r, y in zip(rates[(name, op)], f32)]
            lines.append({"tool": "tools/half_kernels.py --forms", "label": args.label, "kernel": f"{fam} {name} {op}",
                          "peers": P, "bucket_mib": args.mib, "algorithmic_bytes": count * nbytes,
                          "iters_per_pass": args.iters, "passes": PASSES, "rotating_sets": sets,
                          "GB_s_per_pass": [round(r / 1e9, 1) for r in rates[(name, op)]],
                          "bytes_per_s": round(statistics.median(rates[(name, op)])),
                          "GB_s": round(statistics.median(rates[(name, op)]) / 1e9, 1),
                          "ratio_to_f32_per_pass": [round(x, 4) for x in ratios],
                          "ratio_to_f32": round(statistics.median(ratios), 4),
                          "f32_spread": round((max(f32) - min(f32)) / statistics.median(f32), 4),
                          "timing": "two HIP events around back-to-back launches on the library stream"})
        emit(lines, args.out)
        for gs in groups.values():
            for g in gs:
                for b in g:
                    b.free()
        fmi_amd.sync()


def _reduce_acc(alg, P):
    return lambda g, acc: fmi_amd.reduce_tree(Op.SUM, alg, g[P], g[:P], accumulate_f32=acc)


def _scan_acc(alg, P):
    return lambda g, acc: fmi_amd.scan_peers(Op.SUM, alg, g[P:], g[:P], accumulate_f32=acc)


# family: (peers, buckets per group, rotating groups, launch(group, accumulate_f32))
ACC32 = {
    "allreduce8": (8, 9, 3, _reduce_acc(Alg.ALLREDUCE, 8)),
    "scan8": (8, 16, 3, _scan_acc(Alg.SCAN, 8)),
    "reduce_ltr16": (16, 17, 2, _reduce_acc(Alg.REDUCE_LTR, 16)),
    "scan16": (16, 32, 2, _scan_acc(Alg.SCAN, 16)),
}
ACC32_ROWS = [("f32", False), ("bf16", False), ("bf16", True), ("f16", False), ("f16", True)]


def acc32(args):
    nbytes = args.mib * MIB
    for fam in (args.only.split(",") if args.only else list(ACC32)):
        P, count, sets, launch = ACC32[fam]
        groups = {}
        for name, (dt, esz) in DTYPES.items():
            groups[name] = [Bucket.group(count, nbytes // esz, dt) for _ in range(sets)]
            for g in groups[name]:
                for p in range(P):
                    g[p].fill_synthetic(11, p)
        fmi_amd.sync()
        rates = {r: [] for r in ACC32_ROWS}
        for _ in range(PASSES):
            for name, acc in ACC32_ROWS:
                gs = groups[name]
                ms = timed(lambda k: launch(gs[k % len(gs)], acc), args.iters, sets)
                rates[(name, acc)].append(count * nbytes / (ms * 1e-3))
        lines = []
        for name, acc in ACC32_ROWS:
            mine, f32, plain = rates[(name, acc)], rates[("f32", False)], rates[(name, False)]
            spread = lambda xs: round((max(xs) - min(xs)) / statistics.median(xs), 4)  # noqa: E731
            lines.append({"tool": "tools/half_kernels.py --acc32", "label": args.label,
                          "kernel": f"{fam} {name}{' acc32' if acc else ''} sum", "peers": P, "bucket_mib": args.mib,
                          "algorithmic_bytes": count * nbytes, "iters_per_pass": args.iters, "passes": PASSES,
                          "rotating_sets": sets, "GB_s_per_pass": [round(r / 1e9, 1) for r in mine],
                          "GB_s": round(statistics.median(mine) / 1e9, 1), "spread": spread(mine),
                          "ratio_to_plain_per_pass": [round(r / y, 4) for r, y in zip(mine, plain)],
                          "ratio_to_plain": round(statistics.median([r / y for r, y in zip(mine, plain)]), 4),
                          "plain_spread": spread(plain),
                          "ratio_to_f32_per_pass": [round(r / y, 4) for r, y in zip(mine, f32)],
                          "ratio_to_f32": round(statistics.median([r / y for r, y in zip(mine, f32)]), 4),
                          "f32_spread": spread(f32),
                          "timing": "two HIP events around back-to-back launches on the library stream"})
        emit(lines, args.out)
        for gs in groups.values():
            for g in gs:
                for b in g:
                    b.free()
        fmi_amd.sync()


class RawLib:
    """A build of libfmi_dev.so driven through its C-ABI alone (the yardstick library: its own state and stream next to
    the package's library in one process; device pointers are the process's, so both work on the same buckets)."""

    def __init__(self, path):
        import ctypes
        from fmi_amd import _lib
        self.c = ctypes
        self.lib = ctypes.CDLL(path)
        for name in ("fmi_dev_init", "fmi_dev_reduce_tree", "fmi_event_create", "fmi_event_destroy", "fmi_event_record",
                     "fmi_event_sync", "fmi_event_elapsed_ms", "fmi_dev_sync", "fmi_last_error"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name] if name in _lib.SIGNATURES else (ctypes.c_char_p, [])
        self.call("fmi_dev_init", 0)

    def call(self, name, *args):
        rc = getattr(self.lib, name)(*args)
        if rc != 0:
            raise RuntimeError(f"{name}: {rc} {self.lib.fmi_last_error().decode()}")

    def reduce_tree(self, op, dtype, alg, out, ins, n):
        ptrs = (self.c.c_void_p * len(ins))(*[b.ptr for b in ins])
        self.call("fmi_dev_reduce_tree", int(op), int(dtype), int(alg), out.ptr, ptrs, len(ins), 0, n, None)

    def timed(self, launch, iters, warm):
        for k in range(warm):
            launch(k)
        e0, e1, ms = self.c.c_void_p(), self.c.c_void_p(), self.c.c_float()
        self.call("fmi_event_create", self.c.byref(e0))
        self.call("fmi_event_create", self.c.byref(e1))
        self.call("fmi_event_record", e0, None)
        for k in range(warm, warm + iters):
            launch(k)
        self.call("fmi_event_record", e1, None)
        self.call("fmi_event_sync", e1)
        self.call("fmi_event_elapsed_ms", self.c.byref(ms), e0, e1)
        self.call("fmi_event_destroy", e0)
        self.call("fmi_event_destroy", e1)
        return ms.value / iters


# family: (peers, rotating groups, rows (dtype, accumulate_f32))
AVG = {
    "allreduce8": (8, 3, [("f32", False), ("bf16", False), ("bf16", True)]),
    "allreduce16": (16, 2, [("f32", False), ("bf16", False), ("bf16", True)]),
    "allreduce17": (17, 2, [("f32", False)]),
}


def avg(args):
    if not args.yardstick_lib:
        sys.exit("--avg needs --yardstick-lib: the build of libfmi_dev.so whose SUM is the yardstick")
    yard = RawLib(os.path.abspath(args.yardstick_lib))
    nbytes = args.mib * MIB
    spread = lambda xs: round((max(xs) - min(xs)) / statistics.median(xs), 4)  # noqa: E731
    for fam in (args.only.split(",") if args.only else list(AVG)):
        P, sets, rows = AVG[fam]
        count = P + 1
        groups = {}
        for name in {r[0] for r in rows}:
            dt, esz = DTYPES[name]
            groups[name] = [Bucket.group(count, nbytes // esz, dt) for _ in range(sets)]
            for g in groups[name]:
                for p in range(P):
                    g[p].fill_synthetic(11, p)
        fmi_amd.sync()
        mine, base = {r: [] for r in rows}, {r: [] for r in rows}
        for _ in range(PASSES):
            for name, acc in rows:
                gs = groups[name]
                dtype = fmi_amd.device.acc_dtype(gs[0][0].dtype, acc)
                ms = timed(lambda k: fmi_amd.reduce_tree(Op.AVG, Alg.ALLREDUCE, gs[k % sets][P], gs[k % sets][:P],
                                                         accumulate_f32=acc), args.iters, sets)
                mine[(name, acc)].append(count * nbytes / (ms * 1e-3))
                fmi_amd.sync()
                ms = yard.timed(lambda k: yard.reduce_tree(Op.SUM, dtype, Alg.ALLREDUCE, gs[k % sets][P], gs[k % sets][:P],
                                                           gs[0][0].n), args.iters, sets)
                base[(name, acc)].append(count * nbytes / (ms * 1e-3))
                yard.call("fmi_dev_sync")
        lines = []
        for name, acc in rows:
            m, y = mine[(name, acc)], base[(name, acc)]
            line = {"tool": "tools/half_kernels.py --avg", "label": args.label,
                    "kernel": f"{fam} {name}{' acc32' if acc else ''} avg", "peers": P, "bucket_mib": args.mib,
                    "algorithmic_bytes": count * nbytes, "iters_per_pass": args.iters, "passes": PASSES,
                    "rotating_sets": sets, "GB_s_per_pass": [round(r / 1e9, 1) for r in m],
                    "GB_s": round(statistics.median(m) / 1e9, 1), "spread": spread(m),
                    "yardstick": "SUM of the same shape by the yardstick library, same buckets, same passes",
                    "yardstick_GB_s_per_pass": [round(r / 1e9, 1) for r in y],
                    "yardstick_GB_s": round(statistics.median(y) / 1e9, 1), "yardstick_spread": spread(y),
                    "ratio_to_yardstick_per_pass": [round(a / b, 4) for a, b in zip(m, y)],
                    "ratio_to_yardstick": round(statistics.median([a / b for a, b in zip(m, y)]), 4),
                    "yardstick_f32_spread": spread(base[("f32", False)]),
                    "timing": "two HIP events of the launching library around back-to-back launches on its stream"}
            if P > 16:  # SUM kernel + scale kernel: the rates count the SUM's algorithmic bytes for both
                line["launches"] = "the SUM kernel, then the scale kernel in place"
                line["traffic_estimate_ratio"] = round((P + 1) / (P + 3), 4)
            lines.append(line)
        emit(lines, args.out)
        for gs in groups.values():
            for g in gs:
                for b in g:
                    b.free()
        fmi_amd.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256, help="bytes per bucket")
    ap.add_argument("--iters", type=int, default=32, help="timed launches per kernel and pass")
    ap.add_argument("--pair-sets", type=int, default=16)
    ap.add_argument("--tree-sets", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--forms", action="store_true", help="the fused forms (see above) instead of pair / tree8")
    ap.add_argument("--acc32", action="store_true", help="FMI_ACC_F32 beside the plain 16-bit and the f32 kernels")
    ap.add_argument("--avg", action="store_true", help="FMI_OP_AVG beside SUM of the same shape by --yardstick-lib")
    ap.add_argument("--yardstick-lib", default=os.environ.get("FMI_DEV_YARDSTICK_LIB"),
                    help="with --avg: another build of libfmi_dev.so (e.g. the parent commit's) whose SUM is the yardstick")
    ap.add_argument("--only", default=None, help="with --forms / --acc32 / --avg: a comma-separated subset of the families")
    ap.add_argument("--label", default="tree", help="with --forms: what the lines are tagged with (e.g. the commit)")
    args = ap.parse_args()
    fmi_amd.init(0)
    if args.avg:
        return avg(args)
    if args.acc32:
        return acc32(args)
    if args.forms:
        return forms(args)
    nbytes = args.mib * MIB
    P = 8

    pair_sets, groups = {}, {}
    for name, (dt, esz) in DTYPES.items():
        n = nbytes // esz
        pair_sets[name] = [tuple(Bucket(n, dt).fill_synthetic(42 + s, j) for j in range(2)) for s in range(args.pair_sets)]
    for name in ("f32", "bf16"):
        dt, esz = DTYPES[name]
        n = nbytes // esz
        groups[name] = [Bucket.group(P + 1, n, dt) for _ in range(args.tree_sets)]
        for g in groups[name]:
            for p in range(P):
                g[p].fill_synthetic(11, p)
    fmi_amd.sync()

    def pair(name, op):
        sets = pair_sets[name]
        return lambda k: fmi_amd.reduce_pair(op, *sets[k % len(sets)])

    def tree(name):
        gs = groups[name]
        return lambda k: fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, gs[k % len(gs)][P], gs[k % len(gs)][:P])

    # (kernel, family, the f32 yardstick of the family, launch, algorithmic bytes, warm-up launches)
    kernels = [("pair f32 sum", "pair", True, pair("f32", Op.SUM), 3 * nbytes, args.pair_sets),
               ("pair f16 sum", "pair", False, pair("f16", Op.SUM), 3 * nbytes, args.pair_sets),
               ("pair bf16 sum", "pair", False, pair("bf16", Op.SUM), 3 * nbytes, args.pair_sets),
               ("pair bf16 max", "pair", False, pair("bf16", Op.MAX), 3 * nbytes, args.pair_sets),
               ("tree8 f32 sum", "tree8", True, tree("f32"), (P + 1) * nbytes, args.tree_sets),
               ("tree8 bf16 sum", "tree8", False, tree("bf16"), (P + 1) * nbytes, args.tree_sets)]
    rates = {k[0]: [] for k in kernels}
    for _ in range(PASSES):
        for name, _, _, launch, algo, warm in kernels:
            ms = timed(launch, args.iters, warm)
            rates[name].append(algo / (ms * 1e-3))
    yard = {fam: rates[name] for name, fam, is_yard, *_ in kernels if is_yard}
    lines = []
    for name, fam, _, _, algo, _ in kernels:
        f32 = yard[fam]
        ratios = [r / y for r, y in zip(rates[name], f32)]
        lines.append({"tool": "tools/half_kernels.py", "kernel": name, "bucket_mib": args.mib, "algorithmic_bytes": algo,
                      "iters_per_pass": args.iters, "passes": PASSES,
                      "rotating_sets": args.pair_sets if fam == "pair" else args.tree_sets,
                      "GB_s_per_pass": [round(r / 1e9, 1) for r in rates[name]],
                      "bytes_per_s": round(statistics.median(rates[name])),
                      "GB_s": round(statistics.median(rates[name]) / 1e9, 1),
                      "ratio_to_f32_per_pass": [round(x, 4) for x in ratios],
                      "ratio_to_f32": round(statistics.median(ratios), 4),
                      "f32_spread": round((max(f32) - min(f32)) / statistics.median(f32), 4),
                      "timing": "two HIP events around back-to-back launches on the library stream"})
    emit(lines, args.out)


if __name__ == "__main__":
    main()
