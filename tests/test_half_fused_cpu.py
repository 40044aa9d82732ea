"""Guards the fixtures of tests/test_gpu_half_fused.py: at every (P, algorithm, rank / root) that file uses, the
program the kernels run (fmi_schedule_expr, host-only) is the oracle's symbolic expression of the reference
collective, so the values its event-driven simulation produces there are the reference's order. Passes with or
without the 16-bit float kernels; no GPU."""
import re

import pytest

import fmi_amd
from fmi_amd import Alg
from oracle import fmi_oracle as orc
from tests import _half_fused_cases as C


@pytest.mark.parametrize("P", sorted(set(C.LTR_P + C.EXTRA["allreduce_ltr"] + C.EXTRA["scan_ltr"])))
def test_ltr_programs(P):
    # reduce_ltr's root and an ordered allreduce's every rank end with the one left-to-right fold
    assert fmi_amd.schedule_expr(Alg.REDUCE_LTR, P, 0) == orc.expr("reduce", P, root=0, ordered=True)
    assert orc.expr("allreduce", P, rank=P - 1, ordered=True) == orc.expr("reduce", P, root=0, ordered=True)
    for r in sorted({0, 1, P // 2, P - 1}):
        assert fmi_amd.schedule_expr(Alg.SCAN_LTR, P, r) == orc.expr("scan", P, rank=r, ordered=True)


@pytest.mark.parametrize("P", sorted(set(C.REDUCE_P + C.EXTRA["reduce"])))
def test_reduce_programs(P):
    t = fmi_amd.schedule_expr(Alg.REDUCE, P, 0)  # in transformed ids (root -> 0); map back to real ids
    for root in sorted({r % P for r in C.reduce_roots(P)} | {0, P - 1}):
        real = re.sub(r"x(\d+)", lambda m: "x%d" % ((int(m.group(1)) + root) % P), t)
        assert real == orc.expr("reduce", P, root=root)


@pytest.mark.parametrize("P", sorted(set(C.ALLREDUCE_P + C.EXTRA["allreduce"])))
def test_allreduce_programs(P):
    for r in C.allreduce_ranks("max", P):
        assert fmi_amd.schedule_expr(Alg.ALLREDUCE, P, r) == orc.expr("allreduce", P, rank=r)


@pytest.mark.parametrize("P", sorted(set(C.SCAN_P + C.EXTRA["scan"])))
def test_scan_programs(P):
    for r in sorted({0, 1, 15, 16, 17, P // 2, P - 2, P - 1}):
        if 0 <= r < P:
            assert fmi_amd.schedule_expr(Alg.SCAN, P, r) == orc.expr("scan", P, rank=r)


def test_cpp_ordered_host_path_known_answers():
    """fmi_amd/cpp/tests/test_half_ordered.cpp without --gpu: a non-commutative Function on host bf16 buckets gives
    the left-to-right values written out in it, and those are the oracle's with tests/_half.py's combine."""
    import os
    import subprocess

    import numpy as np

    from tests import _half as H

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "build", "cpp", "test_half_ordered")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(root, "fmi_amd", "cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "0 failed checks" in out.stderr, out.stderr[-4000:]
    src = open(os.path.join(root, "fmi_amd", "cpp", "tests", "test_half_ordered.cpp")).read()

    def table(name):
        body = re.search(name + r" = (\{.*?\});", src, re.S).group(1)
        rows = re.findall(r"\{([^{}]*)\}", body)
        return [np.array([int(v, 16) for v in re.findall(r"0x[0-9A-Fa-f]+", row)], np.uint16) for row in rows]

    xs = table("kIn")
    ordered = dict(commutative=False, associative=False)
    for op, ar, sc in (("sum", table("kSumLtr")[0], table("kSumScanLtr")), ("max", table("kMaxLtr")[0], None)):
        f = H.combiner(op, "bf16")
        for got in orc.allreduce(xs, f, **ordered)[0]:
            assert np.array_equal(got, ar)
        if sc is not None:
            for got, want in zip(orc.scan(xs, f, **ordered)[0], sc):
                assert np.array_equal(got, want)
