"""The definition the stochastic-rounding tests compare against (fmi_dev_reduce_tree_mx_sr, fmi_dev_mx_quantize_sr,
fmi_host_mx_quantize_sr; include/fmi_dev.h), restated in numpy.

    S, the block's scale byte e_out and y = fl32(S * 2^(127 - e_out)) are the round-to-nearest calls' (tests/_mx.py,
    tests/_mxfp4.py); only narrow(y) becomes narrow_sr(y, r):
    element i has the stream position j = first + i;  q = j >> 3
    W = Philox4x32-10(counter (q lo, q hi, 0, 0), key (seed lo, seed hi));  r = (W[(j & 7) >> 1] >> 16 (j & 1)) & 0xFFFF
    lo <= |y| < hi neighbours on the type's grid G;  T = 65536 (|y| - lo) / (hi - lo) in float64 (exact);
    the magnitude is hi if r + 0.5 < T, else lo;  |y| == lo stays;  the sign bit is y's

Kinds: "e4m3", "e5m2" (codes are the element bytes) and "e2m1" (codes 0..15, one per element; tests/_mxfp4.pack packs
them). narrow_sr_int is the equal integer form that include/fmi_dev.h states beside the definition; nothing in the
library computes it (the kernels and the host call use exact f32 operations, fmi_amd/csrc/fmi_mx_sr.h, and are compared
with narrow_sr itself), so it is checked here as a second statement of the definition only.
"""
import numpy as np

from tests import _fp8 as F
from tests import _mx as MX
from tests import _mxfp4 as M4

KINDS = ("e4m3", "e5m2", "e2m1")
DTYPE_ID = {"e4m3": 12, "e5m2": 13, "e2m1": 15}
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
# (mantissa bits M, smallest normal exponent EMIN, sign bit of the code, the codes of G)
FORMAT = {"e2m1": (1, 0, 8, 8), "e4m3": (3, -6, 0x80, 0x7F), "e5m2": (2, -14, 0x80, 0x7C)}
SEEDS = (0, 1, 0x0123456789ABCDEF, 2 ** 64 - 1)
FIRSTS = (0, 32, 2 ** 35 - 64)


def grid(kind: str) -> np.ndarray:
    """G: the ascending non-negative finite magnitudes, in float64; the index is the magnitude's code."""
    if kind == "e2m1":
        return M4.MAGNITUDES.astype(np.float64)
    return F.widen(np.arange(FORMAT[kind][3], dtype=np.uint8), kind).astype(np.float64)


def philox(counter, key) -> np.ndarray:
    """Philox4x32-10 over an (n, 4) array of counters and one (k0, k1) key: (n, 4) np.uint32."""
    c = np.asarray(counter, np.uint64).reshape(-1, 4) & MASK
    c0, c1, c2, c3 = (c[:, k].copy() for k in range(4))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # 32 x 32 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def rbits(j, seed: int) -> np.ndarray:
    """r of the stream positions j (u64) under `seed` (u64): np.uint32 values below 65536."""
    j = np.asarray(j, np.uint64).ravel()
    q = j >> np.uint64(3)
    uq, inv = np.unique(q, return_inverse=True)
    zero = np.zeros_like(uq)
    W = philox(np.stack([uq & MASK, uq >> np.uint64(32), zero, zero], axis=1), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    k = (j & np.uint64(7)).astype(np.int64)
    w = W[inv, k >> 1]
    return (w >> (16 * (k & 1)).astype(np.uint32)) & np.uint32(0xFFFF)


def positions(first: int, n: int) -> np.ndarray:
    return np.uint64(first) + np.arange(n, dtype=np.uint64)


def neighbours(y, kind: str):
    """(index of lo, |y| == lo, T) for finite |y| <= max(G); T is 0 where |y| is a grid value."""
    G = grid(kind)
    a = np.abs(np.ascontiguousarray(y, np.float32).astype(np.float64))
    assert np.isfinite(a).all() and (a <= G[-1]).all(), "narrow_sr is defined for finite |y| <= the largest finite element"
    i = np.searchsorted(G, a, side="right") - 1
    lo, hi = G[i], G[np.minimum(i + 1, G.size - 1)]
    exact = a == lo
    T = np.where(exact, 0.0, 65536.0 * (a - lo) / np.where(exact, 1.0, hi - lo))
    return i, exact, T


def narrow_sr(y, r, kind: str) -> np.ndarray:
    """The definition: codes (np.uint8) of y under the 16-bit integers r."""
    y = np.ascontiguousarray(y, np.float32)
    i, exact, T = neighbours(y, kind)
    up = ~exact & (np.asarray(r, np.float64) + 0.5 < T)
    sign = np.where(np.signbit(y), FORMAT[kind][2], 0)
    return ((i + up) | sign).astype(np.uint8)


def narrow_sr_int(y, r, kind: str) -> np.ndarray:
    """The integer form: d = 23 - M + max(EMIN - e, 0); D = sig mod 2^d; up = ((2 r + 1) << (d - 17)) < D."""
    M, emin, signbit, _ = FORMAT[kind]
    u = np.ascontiguousarray(y, np.float32).view(np.uint32).astype(np.int64)
    a = u & 0x7FFFFFFF
    ef = a >> 23
    e = np.maximum(ef, 1) - 127
    sig = (a & 0x7FFFFF) | np.where(ef == 0, 0, 0x800000)
    d = 23 - M + np.maximum(emin - e, 0)
    dd = np.minimum(d, 40)  # sig < 2^24: sig >> d is 0 and D is sig from d = 24 on
    D = sig & ((np.int64(1) << dd) - 1)
    shift = d - 17
    up = (shift < 24) & ((((2 * np.asarray(r, np.int64) + 1)) << np.minimum(shift, 24)) < D)
    code = ((np.maximum(e, emin) - emin) << M) + (sig >> dd) + up
    return (code | np.where(u >> 31, signbit, 0)).astype(np.uint8)


def scaled(S, kind: str):
    """(y, per-element e_out, e_out per block), as the round-to-nearest calls compute them."""
    if kind == "e2m1":
        return M4.scaled(S)
    S = np.ascontiguousarray(S, np.float32)
    e = MX.scale_bytes(S, kind)
    ee = MX.per_element(e, S.size).astype(np.uint32)
    inv = ((np.uint32(254) - np.minimum(ee, 254)) << np.uint32(23)).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        y = (S * inv).astype(np.float32)
    return y, ee, e


def quant_sr(S, kind: str, seed: int, first: int = 0):
    """(codes, scale bytes) of the f32 array S: a block with e_out == 255 stores 0x7F bytes (E2M1: codes 0)."""
    y, ee, e = scaled(S, kind)
    nan = ee == 255
    q = narrow_sr(np.where(nan, np.float32(0), y), rbits(positions(first, y.size), seed), kind)
    return np.where(nan, np.uint8(0 if kind == "e2m1" else 0x7F), q).astype(np.uint8), e


def quant_rne(S, kind: str):
    return M4.quant(S) if kind == "e2m1" else MX.quant(S, kind)


def values(family: str, kind: str, xs, es, op: str = "sum", root: int = 0) -> np.ndarray:
    return M4.values(family, xs, es, op, root) if kind == "e2m1" else MX.values(family, kind, xs, es, op, root)


def expected_sr(family: str, kind: str, xs, es, seed: int, first: int = 0, op: str = "sum", root: int = 0):
    return quant_sr(values(family, kind, xs, es, op, root), kind, seed, first)


def element_bytes(codes, kind: str) -> np.ndarray:
    """The bucket's bytes: the codes themselves, or E2M1 codes packed two to a byte."""
    return M4.pack(codes) if kind == "e2m1" else np.asarray(codes, np.uint8)


def codes_of(raw, kind: str, n: int) -> np.ndarray:
    return M4.unpack(raw, n) if kind == "e2m1" else np.asarray(raw, np.uint8)[:n]


def visible_inputs(kind: str, n: int, P: int, seed: int = 7):
    """The family on which stochastic rounding shows: random finite codes under scale bytes 126..128, so that a sum of P
    peers carries more bits than the element type keeps. A shorter bucket is a prefix of a longer one (per-peer
    streams), so tests cut one draw to their sizes."""
    if kind == "e2m1":
        return M4.random_inputs(n, P, 5000 + seed, 126, 128)
    w = F.widen(np.arange(256, dtype=np.uint8), kind)
    ok = np.flatnonzero(np.isfinite(w)).astype(np.uint8)
    xs = [ok[np.random.default_rng([seed, p, 0]).integers(0, ok.size, n)] for p in range(P)]
    es = [np.random.default_rng([seed, p, 1]).integers(126, 129, MX.blocks(n)).astype(np.uint8) for p in range(P)]
    return xs, es


def cut(xs, es, n: int):
    return [x[:n] for x in xs], [e[:MX.blocks(n)] for e in es]


def max_finite(kind: str) -> np.float32:
    return np.float32(grid(kind)[-1])


def pinned_blocks(vals, kind: str, scale: float = 1.0) -> np.ndarray:
    """f32 blocks of 32 whose first element is the largest finite element times `scale` (a power of two), so that
    e_out = 127 + log2(scale) and y = value / scale; the other 31 elements of every block are taken from vals * scale."""
    vals = np.ascontiguousarray(vals, np.float32)
    nb = -(-vals.size // 31)
    body = np.zeros(nb * 31, np.float32)
    body[:vals.size] = vals
    out = np.empty((nb, 32), np.float32)
    out[:, 0] = max_finite(kind)
    out[:, 1:] = body.reshape(nb, 31)
    return (out.reshape(-1) * np.float32(scale)).astype(np.float32)


def exhaustive_values(kind: str) -> np.ndarray:
    """Every grid value, every midpoint and both f32 neighbours of each, both signs."""
    G = grid(kind)
    mid = (G[:-1] + G[1:]) / 2
    base = np.concatenate([G, mid]).astype(np.float32)
    assert np.array_equal(base.astype(np.float64), np.concatenate([G, mid]))  # all exact in f32
    up, down = np.nextafter(base, np.float32(np.inf)), np.nextafter(base, np.float32(-np.inf))
    v = np.concatenate([base, up, down]).astype(np.float32)
    v = v[(v >= 0) & (v <= max_finite(kind))]
    return np.concatenate([v, -v]).astype(np.float32)
