"""The 16-bit float element types on np.uint16 bit patterns: the definition the half tests compare against.

One combine (include/fmi_dev.h): widen both operands to f32 (exact), apply the op in f32 (IEEE round-to-nearest-
even, subnormals kept), narrow to the storage type (round-to-nearest-even, subnormals kept, NaN stays NaN).
max / min are the reference's selections `(a<b)?b:a` / `(b<a)?b:a`: the kept operand's 16 bits come out unchanged.

kind is "f16" (IEEE binary16) or "bf16" (the upper 16 bits of binary32). Expected values of P-way programs come
from oracle.fmi_oracle's allreduce / reduce / scan with `f` bound to `combiner(op, kind)`: those are generic in `f`
and in the array type, so the event-driven simulation stays the independent check of the schedule.
"""
import numpy as np

from oracle import fmi_oracle as orc

KINDS = ("f16", "bf16")
OPS = ("sum", "prod", "max", "min")


def widen(bits: np.ndarray, kind: str) -> np.ndarray:
    bits = np.asarray(bits, dtype=np.uint16)
    if kind == "f16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def narrow(x: np.ndarray, kind: str) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    if kind == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32)
    lsb = (u >> np.uint32(16)) & np.uint32(1)
    rounded = ((u.astype(np.uint64) + np.uint64(0x7FFF) + lsb) >> np.uint64(16)).astype(np.uint16)
    quiet = ((u >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16)
    return np.where(np.isnan(x), quiet, rounded)


def combine(op: str, a_bits: np.ndarray, b_bits: np.ndarray, kind: str) -> np.ndarray:
    a_bits = np.asarray(a_bits, dtype=np.uint16)
    b_bits = np.asarray(b_bits, dtype=np.uint16)
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
    """`f(mine, received)` for oracle.fmi_oracle's collectives over uint16 bit-pattern buckets."""
    return lambda a, b: combine(op, a, b, kind)


def is_nan(bits: np.ndarray, kind: str) -> np.ndarray:
    return np.isnan(widen(bits, kind))


def from_float(x, kind: str) -> np.ndarray:
    return narrow(np.asarray(x, dtype=np.float32), kind)


def synthetic(kind: str, n: int, seed: int, peer: int, start: int = 0) -> np.ndarray:
    """The synthetic fill restated: f16 = (h >> 53) * 2^-11 * 2 - 1, bf16 = (h >> 56) * 2^-8 * 2 - 1, both exact
    in the storage type and in [-1, 1)."""
    key = np.uint64((seed ^ (peer << 40)) & 0xFFFFFFFFFFFFFFFF)
    h = orc.splitmix64(key ^ np.arange(start, start + n, dtype=np.uint64))
    if kind == "f16":
        u = (h >> np.uint64(53)).astype(np.float32) * np.float32(2.0 ** -11)
    else:
        u = (h >> np.uint64(56)).astype(np.float32) * np.float32(2.0 ** -8)
    v = u * np.float32(2.0) - np.float32(1.0)
    bits = narrow(v, kind)
    assert np.array_equal(widen(bits, kind), v)  # exact in the storage type
    return bits


def edge_values(kind: str) -> np.ndarray:
    """Bit patterns of the edge values the pairwise tests place: each (a[k], b[k]) pair below is one case."""
    if kind == "f16":
        one, max_fin, min_sub, min_norm_q = 0x3C00, 0x7BFF, 0x0001, 0x0100
        small = 0x0C00  # 2^-12: its square 2^-24 is the smallest subnormal
        half = 0x1000  # 2^-11 = half an ulp of 1: added to 1 and to 1 + ulp it ties both ways
    else:
        one, max_fin, min_sub, min_norm_q = 0x3F80, 0x7F7F, 0x0001, 0x0020
        small = 0x1F80  # 2^-64: its square 2^-128 is subnormal
        half = 0x3B80  # 2^-8 = half an ulp of 1
    sign = 0x8000
    inf, nan = (0x7C00, 0x7E00) if kind == "f16" else (0x7F80, 0x7FC0)
    three_half = from_float(widen(np.array([half], np.uint16), kind) * np.float32(3.0), kind)[0]
    a = [0x0000, sign, 0x0000, inf, inf | sign, inf, nan, one, max_fin, max_fin | sign, min_sub, min_norm_q,
         one, one + 1, one, one + 1, max_fin, small, min_sub, min_sub | sign]
    b = [sign, 0x0000, 0x0000, one, one, inf | sign, one, nan, one, one, min_sub, min_norm_q,
         half, half, three_half, three_half, max_fin, small, one, min_sub]
    return np.array(a, np.uint16), np.array(b, np.uint16)


def inputs(kind: str, n: int, seed: int, peer: int):
    """Synthetic fill with the edge values sprinkled in: even peers take the `a` side of every edge pair, odd peers
    the `b` side, at the same indices (spread over the bucket when it holds them all, else its first elements)."""
    x = synthetic(kind, n, seed, peer)
    ea, eb = edge_values(kind)
    e = ea if peer % 2 == 0 else eb
    if n >= 2 * e.size and n % 7919:
        x[(np.arange(e.size) * 7919) % n] = e
    else:
        k = min(n, e.size)
        x[:k] = e[:k]
    return x


def all_patterns(n: int = 1 << 22):
    """a = every 16-bit pattern, 64 times over; b[i] = a[(i * k) mod 65536] for 64 odd k, one per block."""
    assert n % 65536 == 0
    blocks = n // 65536
    base = np.arange(65536, dtype=np.uint32)
    a = np.tile(base.astype(np.uint16), blocks)
    b = np.concatenate([((base * np.uint32(2 * j + 1)) & np.uint32(0xFFFF)).astype(np.uint16) for j in range(blocks)])
    return a, b


def assert_bits(got: np.ndarray, want: np.ndarray, kind: str, op: str, what="") -> None:
    """Raw 16-bit equality; a NaN produced by sum / prod matches any NaN."""
    got = np.asarray(got, np.uint16)
    want = np.asarray(want, np.uint16)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = got == want
    if op in ("sum", "prod"):
        ok |= is_nan(got, kind) & is_nan(want, kind)
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements differ; first at {i}: "
                             f"got 0x{int(got[i]):04x}, want 0x{int(want[i]):04x}")
