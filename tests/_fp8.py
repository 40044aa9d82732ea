"""The 8-bit float element types on np.uint8 bit patterns: the definition the FP8 tests compare against.

kind is "e4m3" (FMI_F8E4M3: OCP E4M3, e4m3fn: bias 7, no infinities, NaN = S.1111.111 only, largest finite 448) or
"e5m2" (FMI_F8E5M2: OCP E5M2: bias 15, IEEE-style infinities and NaNs, largest finite 57344).

widen is exact. narrow rounds to nearest even, keeps subnormals and the zero's sign, and does NOT saturate: a rounded
magnitude beyond the largest finite value (or +-inf) gives +-inf (e5m2) or NaN (e4m3); NaN stays NaN
(include/fmi_dev.h). One combine widens both operands to f32, applies the op in f32 and narrows; max / min are the
reference's selections `(a<b)?b:a` / `(b<a)?b:a` on the widened values and keep the operand's own byte. All of it is
numpy integer code on the bits; tests/test_fp8_cpu.py pins it to torch CPU's float8 tensors.

Expected values of P-way programs come from oracle.fmi_oracle's collectives (generic in `f` and in the array type):
plain programs with `f = combiner(op, kind)` over the bit patterns, FMI_ACC_F32 programs as
tests/_half_acc.py::expected_acc does it, over the widened f32 arrays with its f32_op and narrow on every stored output.
"""
import numpy as np

from oracle import fmi_oracle as orc
from tests._half_acc import f32_op

KINDS = ("e4m3", "e5m2")
OPS = ("sum", "prod", "max", "min")
DTYPE_ID = {"e4m3": 12, "e5m2": 13}
# (mantissa bits, bias, first magnitude (f32 bits) that narrows to inf / NaN outright, the byte it gives)
_FMT = {"e4m3": (3, 7, 0x43F00000, 0x7F), "e5m2": (2, 15, 0x47800000, 0x7C)}
MAX_FINITE = {"e4m3": 448.0, "e5m2": 57344.0}


def _table(kind: str) -> np.ndarray:
    m, bias, _, _ = _FMT[kind]
    b = np.arange(256, dtype=np.int64)
    sign = np.where(b & 0x80, -1.0, 1.0)
    e, f = (b & 0x7F) >> m, (b & ((1 << m) - 1)).astype(np.float64)
    sub = f * 2.0 ** (1 - bias - m)
    nor = (1.0 + f * 2.0 ** -m) * 2.0 ** (e.astype(np.float64) - bias)
    v = np.where(e == 0, sub, nor)
    if kind == "e4m3":
        v = np.where((b & 0x7F) == 0x7F, np.nan, v)
    else:
        v = np.where((b & 0x7F) == 0x7C, np.inf, v)
        v = np.where((b & 0x7F) > 0x7C, np.nan, v)
    return (sign * v).astype(np.float32)


_WIDEN = {k: _table(k) for k in KINDS}


def widen(bits: np.ndarray, kind: str) -> np.ndarray:
    return _WIDEN[kind][np.asarray(bits, dtype=np.uint8)]


def narrow(x: np.ndarray, kind: str) -> np.ndarray:
    m, bias, over, over_byte = _FMT[kind]
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    s, a = (u >> 24) & 0x80, u & 0x7FFFFFFF
    e = (a >> 23) - 127
    emin = 1 - bias
    # normal results: round the f32 mantissa to m bits; a carry runs into the exponent (and, at the top, into the
    # format's own inf / NaN pattern)
    shift = 23 - m
    nor = ((a + ((1 << (shift - 1)) - 1) + ((a >> shift) & 1)) >> shift) - ((127 - bias) << m)
    # subnormal results: the f32 significand shifted down to units of 2^(emin - m), ties to even
    sh = np.clip(shift + (emin - e), shift + 1, 31)
    mant = (a & 0x7FFFFF) | 0x800000
    q, rem, half = mant >> sh, mant & ((1 << sh) - 1), 1 << (sh - 1)
    sub = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    sub = np.where(e < emin - m - 1, 0, sub)  # below half the smallest subnormal (f32 zeros and subnormals too)
    r = np.where(e >= emin, nor, sub)
    r = np.where(a >= over, over_byte, r)
    r = np.where(a > 0x7F800000, 0x7F, r)
    return (s | r).astype(np.uint8)


def is_nan(bits: np.ndarray, kind: str) -> np.ndarray:
    return np.isnan(widen(bits, kind))


def combine(op: str, a_bits: np.ndarray, b_bits: np.ndarray, kind: str) -> np.ndarray:
    a_bits, b_bits = np.asarray(a_bits, dtype=np.uint8), np.asarray(b_bits, dtype=np.uint8)
    a, b = widen(a_bits, kind), widen(b_bits, kind)
    with np.errstate(all="ignore"):
        if op == "sum":
            return narrow(a + b, kind)
        if op == "prod":
            return narrow(a * b, kind)
        if op == "max":
            return np.where(a < b, b_bits, a_bits)
        if op == "min":
            return np.where(b < a, b_bits, a_bits)
    raise ValueError(op)


def combiner(op: str, kind: str):
    """`f(mine, received)` for oracle.fmi_oracle's collectives over uint8 bit-pattern buckets."""
    return lambda a, b: combine(op, a, b, kind)


def synthetic(kind: str, n: int, seed: int, peer: int, start: int = 0) -> np.ndarray:
    """The synthetic fill restated (include/fmi_dev.h): e4m3 = (h >> 60) * 2^-4 * 2 - 1 (multiples of 2^-3),
    e5m2 = (h >> 61) * 2^-3 * 2 - 1 (multiples of 2^-2), both exact in the storage type and in [-1, 1)."""
    key = np.uint64((seed ^ (peer << 40)) & 0xFFFFFFFFFFFFFFFF)
    h = orc.splitmix64(key ^ np.arange(start, start + n, dtype=np.uint64))
    if kind == "e4m3":
        u = (h >> np.uint64(60)).astype(np.float32) * np.float32(2.0 ** -4)
    else:
        u = (h >> np.uint64(61)).astype(np.float32) * np.float32(2.0 ** -3)
    v = u * np.float32(2.0) - np.float32(1.0)
    bits = narrow(v, kind)
    assert np.array_equal(widen(bits, kind), v)  # exact in the storage type
    return bits


def boundary_f32() -> np.ndarray:
    """The 393,216 f32 values whose high 16 bits take every value and whose low 16 bits are one of six: every
    rounding tie of both formats with its two f32 neighbours, every overflow threshold, every subnormal boundary,
    +-0, +-inf and NaNs."""
    hi = np.arange(65536, dtype=np.uint32) << np.uint32(16)
    lo = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)
    return (hi[:, None] | lo[None, :]).reshape(-1).view(np.float32)


def table_pairs():
    """Every (a, b) of the 256 x 256 table: 65,536 elements each."""
    i = np.arange(65536, dtype=np.uint32)
    return (i >> np.uint32(8)).astype(np.uint8), (i & np.uint32(0xFF)).astype(np.uint8)


def acc_values(family: str, kind: str, op: str, xs, root: int = 0):
    """The f32 values of the FMI_ACC_F32 program, not yet narrowed: F32_program(widen(x)), in expected_acc's shapes."""
    ws, f = [widen(x, kind) for x in xs], f32_op(op)
    if family == "allreduce":
        return orc.allreduce(ws, f)[0]
    if family == "allreduce_ltr":
        return orc.allreduce(ws, f, commutative=False, associative=False)[0]
    if family == "reduce":
        return orc.reduce(ws, f, root=root)
    if family == "reduce_ltr":
        return orc.reduce(ws, f, root=0, commutative=False, associative=False)[0]
    if family == "scan":
        return orc.scan(ws, f)[0]
    if family == "scan_ltr":
        return orc.scan(ws, f, commutative=False, associative=False)[0]
    raise ValueError(family)


def expected_acc(family: str, kind: str, op: str, xs, root: int = 0):
    """tests/_half_acc.py::expected_acc for the 8-bit floats: out = narrow(F32_program(widen(x))), every stored
    output narrowed once. allreduce / allreduce_ltr / scan / scan_ltr: a list of bit patterns per rank; reduce:
    (result, every rank's final sendbuf); reduce_ltr: the result."""
    v = acc_values(family, kind, op, xs, root)
    nar = lambda x: narrow(x, kind)  # noqa: E731
    if family == "reduce":
        return nar(v[0]), [nar(s) for s in v[1]]
    if family == "reduce_ltr":
        return nar(v)
    return [nar(x) for x in v]


def mean_of(value_f32: np.ndarray, P: int, kind: str) -> np.ndarray:
    """FMI_OP_AVG's last step: narrow(fl32(S x fl32(1 / P)))."""
    with np.errstate(all="ignore"):
        return narrow(np.asarray(value_f32, np.float32) * (np.float32(1.0) / np.float32(P)), kind)


def expected_plain(family: str, kind: str, op: str, xs, root: int = 0):
    """The plain program: narrowed after every combine, in the program's own order; the shapes of expected_acc."""
    f = combiner(op, kind)
    xs = [np.asarray(x, np.uint8) for x in xs]
    if family == "allreduce":
        return orc.allreduce(xs, f)[0]
    if family == "allreduce_ltr":
        return orc.allreduce(xs, f, commutative=False, associative=False)[0]
    if family == "reduce":
        return orc.reduce(xs, f, root=root)
    if family == "reduce_ltr":
        return orc.reduce(xs, f, root=0, commutative=False, associative=False)[0]
    if family == "scan":
        return orc.scan(xs, f)[0]
    if family == "scan_ltr":
        return orc.scan(xs, f, commutative=False, associative=False)[0]
    raise ValueError(family)


def cancel_inputs(kind: str, n: int, P: int, seed: int):
    """tests/_half_acc.py::cancel_inputs for the 8-bit floats: element i gives one peer +B and another -B; every other
    peer holds a small synthetic value; all of them exact in the format.

    e5m2: B = 2^15, small = synthetic * 2^-12 (multiples of 2^-14 up to 2^-12). B / small >= 2^27, so a small value
    added while a lone +-B is in the f32 partial is absorbed and one added after the pair has cancelled is kept: each
    bracketing gives different bits, and a wrong order cannot hide behind the final rounding.

    e4m3: B = 2^8, small = synthetic * 2^-5 (multiples of 2^-8 up to 2^-5). A SUM cannot show the bracketing on e4m3:
    every e4m3 value is a multiple of 2^-9 below 2^9, so every partial sum of up to 2^10 of them is a multiple of 2^-9
    below 2^19, which f32 holds exactly, and all orders of the f32 program agree. What these inputs tell apart on e4m3 is
    f32 accumulation from the per-combine rounding of the plain dtype, which absorbs every small value next to B. The
    bracketing of the e4m3 kernels is pinned by a PROD instead, through the f32 range: order_inputs below."""
    B = np.float32(2.0 ** 8 if kind == "e4m3" else 2.0 ** 15)
    scale = np.float32(2.0 ** -5 if kind == "e4m3" else 2.0 ** -12)
    i = np.arange(n)
    a = (5 * i + seed) % P
    b = (a + 1 + ((i // P) % (P - 1) if P > 1 else 0)) % P
    xs = []
    for p in range(P):
        v = widen(synthetic(kind, n, seed, p), kind) * scale
        v = np.where(a == p, B, np.where(b == p, -B, v)).astype(np.float32)
        bits = narrow(v, kind)
        assert np.array_equal(widen(bits, kind), v), "cancel_inputs: a value is not exact in the storage type"
        xs.append(bits)
    return xs


def order_inputs(kind: str, n: int, P: int, seed: int):
    """PROD inputs on which the bracketing shows through the f32 RANGE, for both formats, at P = 16: peers 0 .. P-2
    hold +-M (M the largest finite value: 448 = 2^8.8, 57344 = 2^15.8), peer P-1 holds +-0. Left to right the
    product of the first 15 (e4m3; 9 for e5m2) exceeds 2^128 and is inf in f32, and inf x 0 is NaN; the recursive-
    doubling and binomial trees multiply the zero into a partial of at most 8 values (2^70.5; e5m2 2^126.5) and end
    with +-0. In one element of four peer 3 holds 1 (e4m3) or peers 3 .. 9 hold 1 (e5m2), so that no partial leaves
    the range and all orders agree there: a kernel that always gave NaN, or never, fails too."""
    M = np.float32(MAX_FINITE[kind])
    i = np.arange(n)
    calm = i % 4 == 3
    xs = []
    for p in range(P):
        sign = np.where(((i * 7 + p * 13 + seed) // 3) % 2 == 0, np.float32(1), np.float32(-1))
        if p == P - 1:
            v = sign * np.float32(0.0)
        else:
            v = sign * M
            ones = (p == 3) if kind == "e4m3" else (3 <= p <= 9)
            if ones:
                v = np.where(calm, np.float32(1.0), v)
        bits = narrow(v.astype(np.float32), kind)
        assert np.array_equal(widen(bits, kind).view(np.uint32), v.astype(np.float32).view(np.uint32))
        xs.append(bits)
    return xs


def overflow_inputs(kind: str, n: int, P: int, seed: int):
    """Partial sums above the largest finite value that come back in range: peers 0 and 1 hold +M and +M/2 (M the
    largest finite value), peers 2 and 3 hold -M and -M/2, the others a synthetic value. In every order of the five
    algorithms some f32 partial exceeds M; the f32 program's result is the small sum of the others, in range. A
    saturating narrow, or a narrowing after every combine (inf / NaN in a partial), gives other bits."""
    M = np.float32(MAX_FINITE[kind])
    xs = []
    for p in range(P):
        if p < 4:
            v = np.full(n, (M, M / 2, -M, -M / 2)[p], np.float32)
        else:
            v = widen(synthetic(kind, n, seed, p), kind)
        bits = narrow(v, kind)
        assert np.array_equal(widen(bits, kind), v)
        xs.append(bits)
    return xs


def assert_bits(got: np.ndarray, want: np.ndarray, kind: str, what="") -> None:
    """Raw byte equality; a NaN matches any NaN."""
    got, want = np.asarray(got, np.uint8), np.asarray(want, np.uint8)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = (got == want) | (is_nan(got, kind) & is_nan(want, kind))
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements differ; first at {i}: "
                             f"got 0x{int(got[i]):02x}, want 0x{int(want[i]):02x}")
