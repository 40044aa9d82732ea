"""FMI_OP_AVG, the mean over the peers: the definition the avg tests compare against (include/fmi_dev.h).

    out = store( fl_V( S x r_P ) ),   r_P = fl_V(1 / P)

V is f32 for f32 / f16 / bf16 buckets and f64 for f64. S is what the same call with SUM holds in V just before its
store: for the plain dtypes the SUM result itself (f16 / bf16: rounded to storage after every combine, widened
again), with FMI_ACC_F32 the f32 program value, not yet narrowed. So the expected values are oracle.fmi_oracle's
collectives (generic in `f` and in the array type) with tests/_half.py's combine, an np.float32 / np.float64 add,
or tests/_half_acc.py's f32 add over the widened inputs; then ONE numpy multiply by V(1) / V(P), and tests/_half.py's
narrow for the 16-bit types.

kind is "f32", "f64", "f16" or "bf16"; the 16-bit kinds move np.uint16 bit patterns, as in tests/_half.py.
"""
import numpy as np

from oracle import fmi_oracle as orc
from tests import _half as H
from tests import _half_acc as A

KINDS = ("f32", "f64", "f16", "bf16")
NP = {"f32": np.float32, "f64": np.float64}
LANES = {"f32": 4, "f64": 2, "f16": 8, "bf16": 8}  # elements per 16-B lane group


def is_half(kind: str) -> bool:
    return kind in H.KINDS


def sizes(kind: str):
    """A tail alone; one 256-thread tile, one lane group and a ragged tail; several tiles and a tail."""
    L = LANES[kind]
    return [L - 1, 256 * L + L + (L - 1), 4 * 256 * L * 2 + (L - 1)]


def value_type(kind: str):
    return np.float64 if kind == "f64" else np.float32


def reciprocal(kind: str, P: int):
    V = value_type(kind)
    return V(1) / V(P)


def np_add(kind: str):
    T = NP[kind]

    def f(a, b):
        with np.errstate(all="ignore"):
            r = np.asarray(a, T) + np.asarray(b, T)
        assert r.dtype == T
        return r
    return f


def sums(family: str, kind: str, xs, acc32: bool = False, root: int = 0):
    """S in the value type V: allreduce / allreduce_ltr a list per rank, reduce / reduce_ltr one array."""
    if is_half(kind):
        if acc32:
            ins, f, val = [H.widen(x, kind) for x in xs], A.f32_op("sum"), (lambda v: np.asarray(v, np.float32))
        else:
            ins, f, val = list(xs), H.combiner("sum", kind), (lambda v: H.widen(v, kind))
    else:
        assert not acc32, "FMI_ACC_F32 is for the 16-bit float dtypes"
        ins, f, val = [np.asarray(x, NP[kind]) for x in xs], np_add(kind), (lambda v: np.asarray(v, NP[kind]))
    if family == "allreduce":
        return [val(v) for v in orc.allreduce(ins, f)[0]]
    if family == "allreduce_ltr":
        return [val(v) for v in orc.allreduce(ins, f, commutative=False, associative=False)[0]]
    if family == "reduce":
        return val(orc.reduce(ins, f, root=root)[0])
    if family == "reduce_ltr":
        return val(orc.reduce(ins, f, root=0, commutative=False, associative=False)[0])
    raise ValueError(family)


def scale(S, kind: str, P: int):
    """store(fl_V(S x r_P)) of a sum held in V; P = 1 is the copy."""
    V = value_type(kind)
    S = np.asarray(S, V)
    if P == 1:
        y = S
    else:
        with np.errstate(all="ignore"):
            y = S * reciprocal(kind, P)
        assert y.dtype == V
    return H.narrow(y, kind) if is_half(kind) else y


def expected_avg(family: str, kind: str, xs, acc32: bool = False, root: int = 0):
    """The mean of the P = len(xs) buckets in the order of `family`: allreduce / allreduce_ltr a list per rank,
    reduce (at `root`) / reduce_ltr one array. 16-bit kinds: np.uint16 bit patterns."""
    P = len(xs)
    S = sums(family, kind, xs, acc32, root)
    if family in ("allreduce", "allreduce_ltr"):
        return [scale(s, kind, P) for s in S]
    return scale(S, kind, P)


def edge_values(kind: str) -> np.ndarray:
    """f32 / f64: +-0, the smallest and an odd subnormal, the largest finite value, +-inf, NaN, and their negatives."""
    T = NP[kind]
    fi = np.finfo(T)
    sub = fi.smallest_subnormal
    pos = np.array([0.0, sub, sub * 3, sub * 5, fi.tiny, fi.max, np.inf, np.nan, 1.0, 1.0 + fi.eps], T)
    return np.concatenate([pos, -pos]).astype(T)


def inputs(kind: str, n: int, seed: int, peer: int) -> np.ndarray:
    """One peer's bucket. 16-bit kinds: tests/_half.py's inputs. f32 / f64: values of mixed sign over ~40 binades;
    peer 0 carries the edge values at the front, the others -0 there (x + -0 = x, so the SUM keeps every edge value
    and the scaling sees it), and at the end of the bucket, inside its tail."""
    if is_half(kind):
        return H.inputs(kind, n, seed, peer)
    T = NP[kind]
    rng = np.random.default_rng([seed, peer, n])
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(T)
    e = edge_values(kind) if peer == 0 else np.full(edge_values(kind).size, -0.0, T)
    k = min(n, e.size)
    x[:k] = e[:k]
    t = min(n, LANES[kind] - 1)
    if n > e.size + t and t:
        x[n - t:] = e[1:1 + t] if peer == 0 else T(-0.0)
    return x


def assert_same(got, want, kind: str, what: str = "") -> None:
    """Bit-for-bit; a NaN matches any NaN."""
    if is_half(kind):
        H.assert_bits(got, want, kind, "sum", what)
        return
    T = NP[kind]
    U = np.uint32 if kind == "f32" else np.uint64
    got, want = np.asarray(got, T), np.asarray(want, T)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = (got.view(U) == want.view(U)) | (np.isnan(got) & np.isnan(want))
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements differ; first at {i}: "
                             f"got {got[i]!r} (0x{int(got.view(U)[i]):x}), want {want[i]!r} (0x{int(want.view(U)[i]):x})")
