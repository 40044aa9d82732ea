"""The definition the MX reduction tests compare against (fmi_dev_reduce_tree_mx, include/fmi_dev.h): block-scaled
8-bit float buckets, one E8M0 scale byte per 32 elements.

    v_p   = fl32(widen(x_p[i]) * scale32(e_p[i // 32]))
    S     = F32_program_alg(v_0 .. v_{P-1})          tests/_fp8_scaled.py::program
    S     = fl32(S * fl32(1 / P))                     the mean only (tests/_avg.py's reciprocal)
    f32 output:   S
    8-bit output: per block  A = umax bits(|S|);  e_out = scale_byte(A);  out = narrow(fl32(S * 2^(127 - e_out)))

All in np.float32 (one IEEE operation per numpy operation, no contraction) over tests/_fp8.py's widen / narrow.
"""
import numpy as np

from tests import _avg
from tests import _fp8 as F
from tests._fp8_scaled import assert_f32_bits, program

BLOCK = 32
EMAX = {"e4m3": 8, "e5m2": 15}


def blocks(n: int) -> int:
    return (int(n) + BLOCK - 1) // BLOCK


def scale32(e) -> np.ndarray:
    """The f32 value of E8M0 scale bytes: 1..254 -> bits e << 23; 0 -> bits 0x00400000 (2^-127); 255 -> NaN."""
    e = np.asarray(e, np.uint8).astype(np.uint32)
    bits = np.where(e == 0, np.uint32(0x00400000), np.where(e == 255, np.uint32(0x7FC00000), e << np.uint32(23)))
    return bits.astype(np.uint32).view(np.float32)


def per_element(es, n: int) -> np.ndarray:
    """The scale byte of every element: es[i // 32]."""
    es = np.asarray(es, np.uint8)
    assert es.size == blocks(n), (es.size, n)
    return np.repeat(es, BLOCK)[:n]


def dequant(q, es, kind: str) -> np.ndarray:
    """v = fl32(widen(q) * scale32(e)): one f32 multiply."""
    q = np.asarray(q, np.uint8)
    with np.errstate(all="ignore"):
        return (F.widen(q, kind) * scale32(per_element(es, q.size))).astype(np.float32)


def scale_bytes(S, kind: str) -> np.ndarray:
    """e_out per block of the f32 array S (the last block may be ragged: only its existing elements count)."""
    S = np.ascontiguousarray(S, np.float32)
    a = S.view(np.uint32) & np.uint32(0x7FFFFFFF)
    pad = np.zeros(blocks(S.size) * BLOCK, np.uint32)
    pad[:S.size] = a
    A = pad.reshape(-1, BLOCK).max(axis=1).astype(np.int64)
    f, m = A >> 23, A & 0x7FFFFF
    e = np.maximum(f - EMAX[kind] + (m > 0x600000), 0)
    return np.where(f == 255, 255, e).astype(np.uint8)


def quant(S, kind: str):
    """(element bytes, scale bytes) of the f32 array S."""
    S = np.ascontiguousarray(S, np.float32)
    e = scale_bytes(S, kind)
    ee = per_element(e, S.size).astype(np.uint32)
    inv = ((np.uint32(254) - np.minimum(ee, 254)) << np.uint32(23)).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        y = (S * inv).astype(np.float32)
    q = F.narrow(y, kind)
    return np.where(ee == 255, np.uint8(0x7F), q).astype(np.uint8), e


def values(family: str, kind: str, xs, es, op: str = "sum", root: int = 0) -> np.ndarray:
    """S: the f32 program over the dequantized peers, times fl32(1 / P) for the mean."""
    vs = [dequant(x, e, kind) for x, e in zip(xs, es)]
    S = np.asarray(program(family, vs, root) if len(vs) > 1 else vs[0], np.float32)
    if op == "avg":
        with np.errstate(all="ignore"):
            S = (S * _avg.reciprocal("f32", len(vs))).astype(np.float32)
    else:
        assert op == "sum", op
    return S


def expected_mx(family: str, kind: str, xs, es, op: str = "sum", out: str = "same", root: int = 0):
    """(out, out scale bytes or None). out: "same" = an MX bucket of `kind`, "f32" = np.float32 and no scales."""
    S = values(family, kind, xs, es, op, root)
    if out == "f32":
        return S, None
    return quant(S, kind)


def assert_mx(got, got_scales, want, want_scales, kind: str, out: str, what="") -> None:
    """Bits; a NaN element matches any NaN element; scale bytes compare exactly."""
    if out == "f32":
        assert_f32_bits(np.asarray(got).view(np.float32), want, what)
        return
    assert np.array_equal(np.asarray(got_scales, np.uint8), want_scales), \
        f"{what}: scale bytes differ at blocks {np.flatnonzero(np.asarray(got_scales) != want_scales)[:8]}: " \
        f"got {np.asarray(got_scales)[np.asarray(got_scales) != want_scales][:8]}, want {want_scales[np.asarray(got_scales) != want_scales][:8]}"
    F.assert_bits(got, want, kind, what)


def random_inputs(kind: str, n: int, P: int, seed: int, lo: int = 120, hi: int = 134, finite: bool = False):
    """Random non-NaN element bytes and per-block scales drawn per peer from lo..hi, so that peers' blocks are
    misaligned in exponent. E5M2 has two inf bytes among the non-NaN ones, which decide most blocks of a many-peer sum
    (e_out = 255); finite=True leaves them out."""
    rng = np.random.default_rng(seed)
    w = F.widen(np.arange(256, dtype=np.uint8), kind)
    ok = np.flatnonzero(np.isfinite(w) if finite else ~np.isnan(w)).astype(np.uint8)
    xs = [ok[rng.integers(0, ok.size, n)] for _ in range(P)]
    es = [rng.integers(lo, hi + 1, blocks(n)).astype(np.uint8) for _ in range(P)]
    return xs, es
