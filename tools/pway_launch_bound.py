"""Host enqueue cost of the P-way fallbacks: three launch-bound shapes, one per path that takes library scratch (the
blocked walk and the pairwise passes over the arena, the f32 bridge over the f32 temporaries). The buckets are so small
that the host's enqueue is the whole time: a host clock around 200 back-to-back calls ending in a stream synchronise.
An overhead measurement, not a bandwidth one. FMI_DEV_LIB selects another build of the library to compare with.

    python3 tools/pway_launch_bound.py

Prints one JSON line: microseconds per library call (median of 5 repetitions) per shape."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fmi_amd  # noqa: E402
from fmi_amd import Alg, Bucket, DType, Op, Tune, _lib  # noqa: E402

CALLS, REPS = 200, 5


def timed(fn):
    for _ in range(20):
        fn()
    fmi_amd.sync()
    us = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        _lib.call("fmi_stream_sync", None)  # the library stream
        us.append((time.perf_counter() - t0) / CALLS * 1e6)
    return round(statistics.median(us), 2)


def main():
    fmi_amd.init(0)
    rows = {}
    # 1: f32 REDUCE over 1000 peers, n = 131, block launches over arena temporaries
    P, n = 1000, 131
    ins = [Bucket(n, np.float32).fill_synthetic(7, p) for p in range(P)]
    out = Bucket(n, np.float32)
    fmi_amd.tune_set(Tune.BLOCKS_ONE_PASS, 0)
    rows["reduce f32 P=1000 n=131 BLOCKS_ONE_PASS=0 (arena, blocked walk)"] = timed(
        lambda: fmi_amd.reduce_tree(Op.SUM, Alg.REDUCE, out, ins, rank=0))
    fmi_amd.tune_set(Tune.BLOCKS_ONE_PASS, 1)
    # 2: unaligned f32 ALLREDUCE over 40 peers, n = 1000: pairwise passes over arena slots
    P, n = 40, 1000
    whole = [Bucket(n + 1, np.float32).fill_synthetic(7, p) for p in range(P + 1)]
    views = [b.view(1, n) for b in whole]
    rows["allreduce f32 P=40 n=1000 unaligned (arena, stepwise)"] = timed(
        lambda: fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, views[P], views[:P], rank=0))
    # 3: bf16 accumulate_f32 REDUCE over 33 peers, n = 1031: the f32 bridge
    P, n = 33, 1031
    hins = [Bucket(n, DType.BF16).fill_synthetic(7, p) for p in range(P)]
    hout = Bucket(n, DType.BF16)
    rows["reduce bf16 acc32 P=33 n=1031 (f32 bridge)"] = timed(
        lambda: fmi_amd.reduce_tree(Op.SUM, Alg.REDUCE, hout, hins, rank=0, accumulate_f32=True))
    fmi_amd.sync()
    print(json.dumps({"tool": "tools/pway_launch_bound.py", "lib": fmi_amd.LIB_PATH, "calls": CALLS, "reps": REPS, "us_per_call": rows}), flush=True)


if __name__ == "__main__":
    main()
