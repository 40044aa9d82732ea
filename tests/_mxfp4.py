"""The definition the MXFP4 tests compare against (fmi_dev_reduce_tree_mx at FMI_F4E2M1, include/fmi_dev.h):
block-scaled E2M1 buckets, two elements to a byte, one E8M0 scale byte per 32 elements.

    v_p   = fl32(widen(x_p[i]) * scale32(e_p[i // 32]))      widen: the 16-entry table
    S     = F32_program_alg(v_0 .. v_{P-1})                  tests/_fp8_scaled.py::program
    S     = fl32(S * fl32(1 / P))                             the mean only
    f32 output:   S
    E2M1 output:  per block  A = umax bits(|S|);  e_out = scale_byte(A) at EMAX = 2;
                  out = narrow(fl32(S * 2^(127 - e_out))), or every nibble 0 where e_out == 255

Codes are handled one per element (np.uint8, 0..15); pack / unpack move them into and out of the bucket's bytes.
All in np.float32 (one IEEE operation per numpy operation, no contraction).
"""
import numpy as np

from tests import _avg
from tests._fp8_scaled import assert_f32_bits, program
from tests._mx import BLOCK, blocks, per_element, scale32

EMAX = 2
MAGNITUDES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], np.float32)
TABLE = np.concatenate([MAGNITUDES, -MAGNITUDES]).astype(np.float32)  # code 8 is -0
# the seven ties and where they go: the even CODE of the two neighbours
TIES = ((0.25, 0), (0.75, 2), (1.25, 2), (1.75, 4), (2.5, 4), (3.5, 6), (5.0, 6))


def widen(codes) -> np.ndarray:
    return TABLE[np.asarray(codes, np.uint8) & 0xF]


def narrow(y) -> np.ndarray:
    """Round to nearest on the eight magnitudes, ties to the even code, the sign kept. Defined for finite |y| <= 6."""
    y = np.ascontiguousarray(y, np.float32)
    a = np.abs(y)
    assert np.isfinite(a).all() and (a <= 6).all(), "narrow is defined for finite |y| <= 6 only"
    # a midpoint stays below where the lower code is even (>), goes up where the upper code is even (>=)
    c = ((a > np.float32(0.25)).astype(np.uint8) + (a >= np.float32(0.75)) + (a > np.float32(1.25)) + (a >= np.float32(1.75)) +
         (a > np.float32(2.5)) + (a >= np.float32(3.5)) + (a > np.float32(5.0))).astype(np.uint8)
    return (c | (np.signbit(y).astype(np.uint8) << 3)).astype(np.uint8)


def pack(codes) -> np.ndarray:
    """Element 2k in bits 3:0 of byte k, element 2k + 1 in bits 7:4; an odd count leaves the last high nibble 0."""
    c = np.asarray(codes, np.uint8).ravel()
    assert c.size == 0 or c.max() <= 15
    if c.size % 2:
        c = np.concatenate([c, np.zeros(1, np.uint8)])
    return (c[0::2] | (c[1::2] << 4)).astype(np.uint8)


def unpack(packed, n: int) -> np.ndarray:
    b = np.asarray(packed, np.uint8).ravel()
    assert b.size == (n + 1) // 2, (b.size, n)
    out = np.empty(2 * b.size, np.uint8)
    out[0::2], out[1::2] = b & 0xF, b >> 4
    return out[:n]


def dequant(codes, es) -> np.ndarray:
    """v = fl32(widen(x) * scale32(e)): one f32 multiply."""
    codes = np.asarray(codes, np.uint8)
    with np.errstate(all="ignore"):
        return (widen(codes) * scale32(per_element(es, codes.size))).astype(np.float32)


def scale_bytes(S) -> np.ndarray:
    """e_out per block of the f32 array S (the last block may be ragged: only its existing elements count)."""
    S = np.ascontiguousarray(S, np.float32)
    a = S.view(np.uint32) & np.uint32(0x7FFFFFFF)
    pad = np.zeros(blocks(S.size) * BLOCK, np.uint32)
    pad[:S.size] = a
    A = pad.reshape(-1, BLOCK).max(axis=1).astype(np.int64)
    f, m = A >> 23, A & 0x7FFFFF
    e = np.maximum(f - EMAX + (m > 0x400000), 0)
    return np.where(f == 255, 255, e).astype(np.uint8)


def scaled(S):
    """(y, per-element e_out, e_out per block): y = fl32(S * 2^(127 - e_out)), what narrow is fed."""
    S = np.ascontiguousarray(S, np.float32)
    e = scale_bytes(S)
    ee = per_element(e, S.size).astype(np.uint32)
    inv = ((np.uint32(254) - np.minimum(ee, 254)) << np.uint32(23)).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        y = (S * inv).astype(np.float32)
    return y, ee, e


def quant(S):
    """(codes, scale bytes) of the f32 array S. A block with an inf or a NaN: byte 255 and every code 0."""
    y, ee, e = scaled(S)
    nan = ee == 255
    q = narrow(np.where(nan, np.float32(0), y))
    return np.where(nan, np.uint8(0), q).astype(np.uint8), e


def values(family: str, xs, es, op: str = "sum", root: int = 0) -> np.ndarray:
    vs = [dequant(x, e) for x, e in zip(xs, es)]
    S = np.asarray(program(family, vs, root) if len(vs) > 1 else vs[0], np.float32)
    if op == "avg":
        with np.errstate(all="ignore"):
            S = (S * _avg.reciprocal("f32", len(vs))).astype(np.float32)
    else:
        assert op == "sum", op
    return S


def expected(family: str, xs, es, op: str = "sum", out: str = "same", root: int = 0):
    """(out, out scale bytes or None). out: "same" = E2M1 codes (one per element), "f32" = np.float32, no scales."""
    S = values(family, xs, es, op, root)
    if out == "f32":
        return S, None
    return quant(S)


def assert_mx(got, got_scales, want, want_scales, out: str, what="") -> None:
    """f32: bits, a NaN matches any NaN. E2M1: codes and scale bytes compare exactly."""
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
    """Codes drawn from all 16 nibbles and per-block scales drawn per peer from lo..hi. Every peer's codes and scale
    bytes come from streams of their own, keyed by (seed, peer), so a shorter bucket is a PREFIX of a longer one of the
    same seed: random_inputs(m, ...) equals random_inputs(n, ...) cut to m elements and blocks(m) scale bytes
    (tests/test_mxfp4_cpu.py asserts it)."""
    xs = [np.random.default_rng([seed, p, 0]).integers(0, 16, n).astype(np.uint8) for p in range(P)]
    es = [np.random.default_rng([seed, p, 1]).integers(lo, hi + 1, blocks(n)).astype(np.uint8) for p in range(P)]
    return xs, es


# The order cases: what tests/test_gpu_mxfp4.py runs at scale bytes 112..142 with an f32 output, and what
# tests/test_mxfp4_cpu.py asserts the bracketings to differ on. With scale bytes in 120..134 every partial sum is exact
# in f32 and no bracketing can show. The GPU test draws order_inputs(P, N_FUSED) and cuts it to its sizes, which by the
# prefix property are order_inputs(P, n) themselves.
N_TILE = 256 * 32 + 96 + 17  # one whole 256-lane tile, three more blocks and an odd ragged tail of 17
ORDER_RANGE = (112, 142)
ORDER_PEERS = (8, 13, 16)


def order_inputs(P: int, n: int = N_TILE):
    return random_inputs(n, P, 1000 + P, *ORDER_RANGE)
