"""The definition the MXFP6 tests compare against (fmi_dev_reduce_tree_mx at FMI_F6E2M3 / FMI_F6E3M2 and the
stochastic-rounding calls at those types, include/fmi_dev.h): block-scaled 6-bit float buckets, four elements to three
bytes, one E8M0 scale byte per 32 elements.

    v_p   = fl32(widen(x_p[i]) * scale32(e_p[i // 32]))      widen: the 64-entry table
    S     = F32_program_alg(v_0 .. v_{P-1})                  tests/_fp8_scaled.py::program
    S     = fl32(S * fl32(1 / P))                             the mean only
    f32 output:   S
    FP6 output:   per block  A = umax bits(|S|);  e_out = scale_byte(A);
                  out = narrow(fl32(S * 2^(127 - e_out))), or every code 0 where e_out == 255

Kinds: "e2m3" and "e3m2". Codes are handled one per element (np.uint8, 0..63); pack / unpack move them into and out of
the bucket's bytes. All in np.float32 (one IEEE operation per numpy operation, no contraction). narrow_sr is the
definition of the stochastic rounding on the two grids, narrow_sr_int its integer restatement; both take their random
bits from tests/_mx_sr.py's philox / rbits.
"""
import numpy as np

from tests import _avg
from tests import _mx_sr as SR
from tests._fp8_scaled import assert_f32_bits, program
from tests._mx import BLOCK, blocks, per_element, scale32

KINDS = ("e2m3", "e3m2")
DTYPE_ID = {"e2m3": 16, "e3m2": 17}
# (mantissa bits M, exponent bias, smallest normal exponent EMIN, EMAX of the scale rule, the largest element's mantissa)
FORMAT = {"e2m3": (3, 1, 0, 2, 0x700000), "e3m2": (2, 3, -2, 4, 0x600000)}
SIGN = 0x20


def _magnitudes(kind: str) -> np.ndarray:
    M, bias, _, _, _ = FORMAT[kind]
    c = np.arange(32)
    e, m = c >> M, c & ((1 << M) - 1)
    v = np.where(e == 0, m / 2.0 ** M * 2.0 ** (1 - bias), (1 + m / 2.0 ** M) * 2.0 ** (e - bias))
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)
    return out


MAGNITUDES = {k: _magnitudes(k) for k in KINDS}
TABLE = {k: np.concatenate([MAGNITUDES[k], -MAGNITUDES[k]]).astype(np.float32) for k in KINDS}  # code 0x20 is -0
MAX = {k: np.float32(MAGNITUDES[k][-1]) for k in KINDS}  # 7.5, 28


def ties(kind: str):
    """The 31 midpoints and where they go: the even CODE of the two neighbours."""
    G = MAGNITUDES[kind].astype(np.float64)
    return tuple((np.float32((G[c] + G[c + 1]) / 2), c if c % 2 == 0 else c + 1) for c in range(31))


def widen(codes, kind: str) -> np.ndarray:
    return TABLE[kind][np.asarray(codes, np.uint8) & 0x3F]


def narrow(y, kind: str) -> np.ndarray:
    """Round to nearest on the 32 magnitudes, ties to the even code, the sign kept. Defined for finite |y| <= MAX."""
    y = np.ascontiguousarray(y, np.float32)
    a = np.abs(y).astype(np.float64)
    G = MAGNITUDES[kind].astype(np.float64)
    assert np.isfinite(a).all() and (a <= G[-1]).all(), "narrow is defined for finite |y| <= the largest element only"
    lo = np.searchsorted(G, a, side="right") - 1
    hi = np.minimum(lo + 1, 31)
    dl, dh = a - G[lo], G[hi] - a  # exact in float64
    up = (lo != hi) & ((dh < dl) | ((dh == dl) & (lo % 2 == 1)))
    return ((lo + up) | (np.signbit(y).astype(np.int64) << 5)).astype(np.uint8)


def nbytes(n: int) -> int:
    return (3 * n + 3) // 4


def pack(codes) -> np.ndarray:
    """Element i in bits 6 i .. 6 i + 5 of the little-endian bit string; the last byte's unused high bits are 0."""
    c = np.asarray(codes, np.uint8).ravel()
    assert c.size == 0 or c.max() <= 63
    bits = ((c[:, None] >> np.arange(6, dtype=np.uint8)) & 1).astype(np.uint8).ravel()
    return np.packbits(bits, bitorder="little")


def unpack(packed, n: int) -> np.ndarray:
    b = np.asarray(packed, np.uint8).ravel()
    assert b.size == nbytes(n), (b.size, n)
    bits = np.unpackbits(b, bitorder="little")[:6 * n].reshape(n, 6)
    return (bits << np.arange(6, dtype=np.uint8)).sum(axis=1).astype(np.uint8)


def dequant(codes, es, kind: str) -> np.ndarray:
    """v = fl32(widen(x) * scale32(e)): one f32 multiply."""
    codes = np.asarray(codes, np.uint8)
    with np.errstate(all="ignore"):
        return (widen(codes, kind) * scale32(per_element(es, codes.size))).astype(np.float32)


def scale_bytes(S, kind: str) -> np.ndarray:
    """e_out per block of the f32 array S (the last block may be ragged: only its existing elements count)."""
    _, _, _, emax, mant = FORMAT[kind]
    S = np.ascontiguousarray(S, np.float32)
    a = S.view(np.uint32) & np.uint32(0x7FFFFFFF)
    pad = np.zeros(blocks(S.size) * BLOCK, np.uint32)
    pad[:S.size] = a
    A = pad.reshape(-1, BLOCK).max(axis=1).astype(np.int64)
    f, m = A >> 23, A & 0x7FFFFF
    e = np.maximum(f - emax + (m > mant), 0)
    return np.where(f == 255, 255, e).astype(np.uint8)


def scaled(S, kind: str):
    """(y, per-element e_out, e_out per block): y = fl32(S * 2^(127 - e_out)), what narrow is fed."""
    S = np.ascontiguousarray(S, np.float32)
    e = scale_bytes(S, kind)
    ee = per_element(e, S.size).astype(np.uint32)
    inv = ((np.uint32(254) - np.minimum(ee, 254)) << np.uint32(23)).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        y = (S * inv).astype(np.float32)
    return y, ee, e


def quant(S, kind: str):
    """(codes, scale bytes) of the f32 array S. A block with an inf or a NaN: byte 255 and every code 0."""
    y, ee, e = scaled(S, kind)
    nan = ee == 255
    q = narrow(np.where(nan, np.float32(0), y), kind)
    return np.where(nan, np.uint8(0), q).astype(np.uint8), e


def values(family: str, kind: str, xs, es, op: str = "sum", root: int = 0) -> np.ndarray:
    vs = [dequant(x, e, kind) for x, e in zip(xs, es)]
    S = np.asarray(program(family, vs, root) if len(vs) > 1 else vs[0], np.float32)
    if op == "avg":
        with np.errstate(all="ignore"):
            S = (S * _avg.reciprocal("f32", len(vs))).astype(np.float32)
    else:
        assert op == "sum", op
    return S


def expected(family: str, kind: str, xs, es, op: str = "sum", out: str = "same", root: int = 0):
    """(out, out scale bytes or None). out: "same" = FP6 codes (one per element), "f32" = np.float32, no scales."""
    S = values(family, kind, xs, es, op, root)
    if out == "f32":
        return S, None
    return quant(S, kind)


def assert_mx(got, got_scales, want, want_scales, out: str, what="") -> None:
    """f32: bits, a NaN matches any NaN. FP6: codes and scale bytes compare exactly."""
    if out == "f32":
        assert_f32_bits(np.asarray(got).view(np.float32), want, what)
        return
    gs = np.asarray(got_scales, np.uint8)
    bad = np.flatnonzero(gs != want_scales)
    assert bad.size == 0, f"{what}: scale bytes differ at blocks {bad[:8]}: got {gs[bad[:8]]}, want {want_scales[bad[:8]]}"
    g = np.asarray(got, np.uint8)
    assert g.shape == want.shape, (what, g.shape, want.shape)
    bad = np.flatnonzero(g != want)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} codes differ; first at {bad[:8]}: got {g[bad[:8]]}, want {want[bad[:8]]}"


def random_inputs(n: int, P: int, seed: int, lo: int = 120, hi: int = 134):
    """Codes drawn from all 64 and per-block scales drawn per peer from lo..hi. Every peer's codes and scale bytes come
    from streams of their own, keyed by (seed, peer), so a shorter bucket is a PREFIX of a longer one of the same seed."""
    xs = [np.random.default_rng([seed, p, 0]).integers(0, 64, n).astype(np.uint8) for p in range(P)]
    es = [np.random.default_rng([seed, p, 1]).integers(lo, hi + 1, blocks(n)).astype(np.uint8) for p in range(P)]
    return xs, es


# The order cases: scale bytes 112..142 with an f32 output; with scale bytes in 120..134 every partial sum is exact in
# f32 and no bracketing can show.
ORDER_SIZES = (8305, 12295)
ORDER_RANGE = (112, 142)
EXACT_RANGE = (120, 134)
ORDER_PEERS = (8, 13, 16)
# one 256-lane tile of the fused kernel (two blocks per lane)
TILE = 256 * 64
SIZES = (1, 3, 31, 32, 33, 63, 64, 65) + tuple(TILE + 96 + r for r in (17, 18, 19, 20))


def order_inputs(P: int, n: int = ORDER_SIZES[-1], rng=ORDER_RANGE):
    return random_inputs(n, P, 1000 + P, *rng)


# ---- stochastic rounding ---------------------------------------------------------------------------------------------
def sr_neighbours(y, kind: str):
    G = MAGNITUDES[kind].astype(np.float64)
    a = np.abs(np.ascontiguousarray(y, np.float32).astype(np.float64))
    assert np.isfinite(a).all() and (a <= G[-1]).all(), "narrow_sr is defined for finite |y| <= the largest element"
    i = np.searchsorted(G, a, side="right") - 1
    lo, hi = G[i], G[np.minimum(i + 1, 31)]
    exact = a == lo
    T = np.where(exact, 0.0, 65536.0 * (a - lo) / np.where(exact, 1.0, hi - lo))
    return i, exact, T


def narrow_sr(y, r, kind: str) -> np.ndarray:
    """The definition: the magnitude is hi if r + 0.5 < T, else lo; a grid value stays; the sign bit is y's."""
    y = np.ascontiguousarray(y, np.float32)
    i, exact, T = sr_neighbours(y, kind)
    up = ~exact & (np.asarray(r, np.float64) + 0.5 < T)
    return ((i + up) | np.where(np.signbit(y), SIGN, 0)).astype(np.uint8)


def narrow_sr_int(y, r, kind: str) -> np.ndarray:
    """The integer form: d = 23 - M + max(EMIN - e, 0); D = sig mod 2^d; up = ((2 r + 1) << (d - 17)) < D."""
    M, _, emin, _, _ = FORMAT[kind]
    u = np.ascontiguousarray(y, np.float32).view(np.uint32).astype(np.int64)
    a = u & 0x7FFFFFFF
    ef = a >> 23
    e = np.maximum(ef, 1) - 127
    sig = (a & 0x7FFFFF) | np.where(ef == 0, 0, 0x800000)
    d = 23 - M + np.maximum(emin - e, 0)
    dd = np.minimum(d, 40)
    D = sig & ((np.int64(1) << dd) - 1)
    shift = d - 17
    up = (shift < 24) & ((((2 * np.asarray(r, np.int64) + 1)) << np.minimum(shift, 24)) < D)
    code = ((np.maximum(e, emin) - emin) << M) + (sig >> dd) + up
    return (code | np.where(u >> 31, SIGN, 0)).astype(np.uint8)


def quant_sr(S, kind: str, seed: int, first: int = 0):
    """(codes, scale bytes) of the f32 array S under stochastic rounding: the round-to-nearest call's scale bytes."""
    y, ee, e = scaled(S, kind)
    nan = ee == 255
    q = narrow_sr(np.where(nan, np.float32(0), y), SR.rbits(SR.positions(first, y.size), seed), kind)
    return np.where(nan, np.uint8(0), q).astype(np.uint8), e


def expected_sr(family: str, kind: str, xs, es, seed: int, first: int = 0, op: str = "sum", root: int = 0):
    return quant_sr(values(family, kind, xs, es, op, root), kind, seed, first)


def visible_inputs(kind: str, n: int, P: int, seed: int = 7):
    """Random codes under scale bytes 125..128: a sum of P peers carries more bits than the element type keeps."""
    return random_inputs(n, P, 5000 + seed, 125, 128)


def exhaustive_values(kind: str) -> np.ndarray:
    """Every grid value, every midpoint and both f32 neighbours of each, halves of the smallest subnormal, both signs
    (+-0 among them)."""
    G = MAGNITUDES[kind].astype(np.float64)
    mid = (G[:-1] + G[1:]) / 2
    base = np.concatenate([G, mid, [G[1] / 4, G[1] / 2 * 0.999]]).astype(np.float32)
    up, down = np.nextafter(base, np.float32(np.inf)), np.nextafter(base, np.float32(-np.inf))
    v = np.concatenate([base, up, down]).astype(np.float32)
    v = v[(v >= 0) & (v <= MAX[kind])]
    return np.concatenate([v, -v]).astype(np.float32)


def pinned_blocks(vals, kind: str) -> np.ndarray:
    """f32 blocks of 32 whose element 0 is the type's largest value, so e_out = 127, the inverse scale is 1 and y is the
    value itself; the other 31 elements of every block are taken from vals."""
    vals = np.ascontiguousarray(vals, np.float32)
    nb = -(-vals.size // 31)
    body = np.zeros(nb * 31, np.float32)
    body[:vals.size] = vals
    out = np.empty((nb, 32), np.float32)
    out[:, 0] = MAX[kind]
    out[:, 1:] = body.reshape(nb, 31)
    return out.reshape(-1)
