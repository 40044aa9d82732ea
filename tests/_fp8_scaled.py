"""The definition the scaled FP8 reduction tests compare against (fmi_dev_reduce_tree_scaled, include/fmi_dev.h):

    v_p  = fl32(widen(x_p) * s_p)
    S    = F32_program_alg(v_0 .. v_{P-1})        the oracle's collectives over f32 arrays, tests/_fp8.py::acc_values' way
    amax = max over the elements of bits(|S|) as unsigned integers
    out  = narrow(fl32(S * t)) or fl32(S * t)

All in np.float32 (one IEEE operation per numpy operation, no contraction) over tests/_fp8.py's widen / narrow.
"""
import numpy as np

from oracle import fmi_oracle as orc
from tests import _fp8 as F
from tests._half_acc import f32_op

FAMILIES = ("allreduce", "reduce", "reduce_ltr")
T_OUT = np.float32(0.7123)


def scales(P: int) -> np.ndarray:
    """s_p = f32((1 + (0.37 p mod 1)) / 3 * 2^((p mod 5) - 2)): a different inexact multiplier per peer."""
    p = np.arange(P, dtype=np.float64)
    return ((1.0 + np.mod(0.37 * p, 1.0)) / 3.0 * 2.0 ** (np.mod(p, 5) - 2)).astype(np.float32)


def scaled_values(kind: str, xs, s) -> list:
    s = np.asarray(s, np.float32)
    with np.errstate(all="ignore"):
        return [(F.widen(x, kind) * s[p]).astype(np.float32) for p, x in enumerate(xs)]


def program(family: str, vs, root: int = 0) -> np.ndarray:
    """The f32 SUM program of `family` over the f32 arrays vs: the result a reduction call stores (rank 0's for an
    allreduce: a sum's bits are every rank's)."""
    f = f32_op("sum")
    if family == "allreduce":
        return orc.allreduce(vs, f)[0][0]
    if family == "allreduce_ltr":
        return orc.allreduce(vs, f, commutative=False, associative=False)[0][0]
    if family == "reduce":
        return orc.reduce(vs, f, root=root)[0]
    if family == "reduce_ltr":
        return orc.reduce(vs, f, root=0, commutative=False, associative=False)[0]
    raise ValueError(family)


def amax_bits(S: np.ndarray) -> int:
    return int(np.abs(np.asarray(S, np.float32)).view(np.uint32).max())


def expected_scaled(family: str, kind: str, xs, s, t, out: str, root: int = 0):
    """(out, amax bits, S). out: "same" = bytes of `kind`, "f32" = np.float32. t: the output scale, None = 1."""
    S = np.asarray(program(family, scaled_values(kind, xs, s), root), np.float32)
    with np.errstate(all="ignore"):
        y = (S * np.float32(1.0 if t is None else t)).astype(np.float32)
    return (F.narrow(y, kind) if out == "same" else y), amax_bits(S), S


def fold_amax(old_bits: int, new_bits: int) -> int:
    return max(int(old_bits), int(new_bits))


def assert_f32_bits(got: np.ndarray, want: np.ndarray, what="") -> None:
    """uint32 equality; a NaN matches any NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements differ; first at {i}: "
                             f"got 0x{int(got.view(np.uint32)[i]):08x}, want 0x{int(want.view(np.uint32)[i]):08x}")


def assert_amax(got_bits: int, want_bits: int, what="") -> None:
    nan = lambda b: (int(b) & 0x7FFFFFFF) > 0x7F800000  # noqa: E731
    assert int(got_bits) == int(want_bits) or (nan(got_bits) and nan(want_bits)), \
        f"{what}: amax 0x{int(got_bits):08x}, want 0x{int(want_bits):08x}"


def assert_out(got, want, kind: str, out: str, what="") -> None:
    if out == "same":
        F.assert_bits(got, want, kind, what)
    else:
        assert_f32_bits(np.asarray(got).view(np.float32), want, what)
