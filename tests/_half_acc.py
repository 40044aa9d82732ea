"""FMI_ACC_F32 on the 16-bit float buckets: the definition the acc32 tests compare against.

A P-way program at `T | FMI_ACC_F32` (include/fmi_dev.h) widens every input to f32, runs the same program in the
same order with f32 combines, and narrows every value it stores to T once: out = narrow(F32_program(widen(x))).
So the expected values are oracle.fmi_oracle's collectives (generic in `f` and in the array type) over the widened
f32 arrays with `f` an np.float32 add / multiply, and tests/_half.py's narrow on every stored output.
"""
import numpy as np

from oracle import fmi_oracle as orc
from tests import _half as H

FAMILIES = ("allreduce", "allreduce_ltr", "reduce", "reduce_ltr", "scan", "scan_ltr")


def f32_op(op: str):
    def f(a, b):
        a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
        with np.errstate(all="ignore"):
            r = a + b if op == "sum" else a * b
        assert r.dtype == np.float32
        return r
    if op not in ("sum", "prod"):
        raise ValueError(f"f32 accumulation changes sum and prod alone, not {op}")
    return f


def expected_acc(family: str, kind: str, op: str, xs, root: int = 0):
    """allreduce / allreduce_ltr / scan / scan_ltr: a list of bit patterns per rank; reduce: (result, every rank's
    final sendbuf); reduce_ltr: the result."""
    ws, f = [H.widen(x, kind) for x in xs], f32_op(op)
    nar = lambda v: H.narrow(v, kind)  # noqa: E731
    if family == "allreduce":
        return [nar(v) for v in orc.allreduce(ws, f)[0]]
    if family == "allreduce_ltr":
        return [nar(v) for v in orc.allreduce(ws, f, commutative=False, associative=False)[0]]
    if family == "reduce":
        res, sends = orc.reduce(ws, f, root=root)
        return nar(res), [nar(s) for s in sends]
    if family == "reduce_ltr":
        return nar(orc.reduce(ws, f, root=0, commutative=False, associative=False)[0])
    if family == "scan":
        return [nar(v) for v in orc.scan(ws, f)[0]]
    if family == "scan_ltr":
        return [nar(v) for v in orc.scan(ws, f, commutative=False, associative=False)[0]]
    raise ValueError(family)


def cancel_inputs(kind: str, n: int, P: int, seed: int):
    """Inputs for which the BRACKETING decides the rounded result (H.inputs alone cannot show a wrong order: the
    final rounding hides it). Element i gives one peer +B and another -B, B = 2^15 (f16) / 2^40 (bf16); every other
    peer holds a synthetic value scaled by 2^-12. A small value added while a lone +-B is in the partial is absorbed
    in f32, one added after the pair has cancelled is kept: each order gives different bits."""
    B = np.float32(2.0 ** 15 if kind == "f16" else 2.0 ** 40)
    i = np.arange(n)
    a = (5 * i + seed) % P
    b = (a + 1 + ((i // P) % (P - 1) if P > 1 else 0)) % P
    xs = []
    for p in range(P):
        v = H.widen(H.synthetic(kind, n, seed, p), kind) * np.float32(2.0 ** -12)
        v = np.where(a == p, B, np.where(b == p, -B, v)).astype(np.float32)
        bits = H.narrow(v, kind)
        assert np.array_equal(H.widen(bits, kind), v), "cancel_inputs: a value is not exact in the storage type"
        xs.append(bits)
    return xs


def differing(a, b, kind: str) -> float:
    """Fraction of the elements that are no NaN in either array at which the bits differ."""
    a, b = np.asarray(a, np.uint16), np.asarray(b, np.uint16)
    ok = ~(H.is_nan(a, kind) | H.is_nan(b, kind))
    return float((a[ok] != b[ok]).mean())
