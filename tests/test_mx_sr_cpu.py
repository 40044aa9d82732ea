"""Stochastic rounding without a GPU: the numpy definition (tests/_mx_sr.py) against its own known answers and its
integer form, and fmi_host_mx_quantize_sr (the C++ functions the kernels share, on host memory) against the definition,
bit for bit; the host-side argument checks of the four calls."""
import ctypes

import numpy as np
import pytest

import fmi_amd
from fmi_amd import _lib
from tests import _fp8 as F
from tests import _mx as MX
from tests import _mx_sr as SR
from tests import _mxfp4 as M4

KNOWN = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)
R_EDGES = (0, 1, 32767, 32768, 65534, 65535)


def test_philox_known_answers():
    for counter, key, want in KNOWN:
        assert tuple(int(x) for x in SR.philox([counter], key)[0]) == want, (counter, key)
    # many counters at once equal one at a time
    cs = np.random.default_rng(0).integers(0, 2 ** 32, (64, 4))
    assert np.array_equal(SR.philox(cs, (5, 7)), np.concatenate([SR.philox([c], (5, 7)) for c in cs]))


@pytest.mark.parametrize("seed", SR.SEEDS)
def test_r_of_an_element_is_16_bits_of_its_group(seed):
    key = (seed & 0xFFFFFFFF, seed >> 32)
    # across one group of 8: word (j & 7) >> 1, the low half for an even j
    for q in (0, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 61 - 1):
        W = SR.philox([(q & 0xFFFFFFFF, q >> 32, 0, 0)], key)[0]
        want = [(int(W[k >> 1]) >> (16 * (k & 1))) & 0xFFFF for k in range(8)]
        assert [int(x) for x in SR.rbits(np.uint64(8 * q) + np.arange(8, dtype=np.uint64), seed)] == want, q
    # across q = 2^32 - 1 -> 2^32: the counter's second word takes the carry
    j = np.uint64(2 ** 35 - 8) + np.arange(16, dtype=np.uint64)
    lo, hi = SR.philox([(0xFFFFFFFF, 0, 0, 0)], key)[0], SR.philox([(0, 1, 0, 0)], key)[0]
    want = [(int(W[k >> 1]) >> (16 * (k & 1))) & 0xFFFF for W in (lo, hi) for k in range(8)]
    assert [int(x) for x in SR.rbits(j, seed)] == want
    assert not np.array_equal(lo, hi)


def in_range(kind):
    """The f32 boundary set of the FP8 / MXFP4 tests cut to narrow_sr's domain (f32 subnormals included), with every
    grid value, every midpoint and their f32 neighbours."""
    b = F.boundary_f32()
    b = b[np.isfinite(b) & (np.abs(b) <= SR.max_finite(kind))]
    sub = (np.arange(1, 4096, dtype=np.uint32) * np.uint32(2047)).view(np.float32)  # f32 subnormals
    return np.concatenate([b, sub, -sub, SR.exhaustive_values(kind)]).astype(np.float32)


@pytest.mark.parametrize("kind", SR.KINDS)
def test_integer_form_equals_the_exact_form(kind):
    y = in_range(kind)
    assert (np.abs(y[y != 0]).min() < 1e-40) and np.isin(SR.grid(kind).astype(np.float32), y).all()
    for r in R_EDGES:
        rr = np.full(y.size, r)
        assert np.array_equal(SR.narrow_sr(y, rr, kind), SR.narrow_sr_int(y, rr, kind)), (kind, r)
    rr = np.random.default_rng(1).integers(0, 65536, y.size)
    assert np.array_equal(SR.narrow_sr(y, rr, kind), SR.narrow_sr_int(y, rr, kind)), kind


@pytest.mark.parametrize("kind", SR.KINDS)
def test_output_is_a_neighbour_and_grid_values_never_move(kind):
    G = SR.grid(kind)
    y = in_range(kind)
    a = np.abs(y.astype(np.float64))
    lo = np.searchsorted(G, a, side="right") - 1
    rr = np.random.default_rng(2).integers(0, 65536, y.size)
    mag = SR.narrow_sr(y, rr, kind) & (SR.FORMAT[kind][2] - 1)
    assert ((mag == lo) | ((mag == lo + 1) & (G[lo] != a))).all()
    assert np.array_equal(SR.narrow_sr(y, rr, kind) >= SR.FORMAT[kind][2], np.signbit(y))  # the sign bit is y's, -0 included
    # grid values, both signs, under 16 seeds: the code of the value itself, which is what round-to-nearest gives
    g = np.concatenate([G, -G]).astype(np.float32)
    S = SR.pinned_blocks(g, kind)
    rne, _ = SR.quant_rne(S, kind)
    for seed in range(16):
        q, e = SR.quant_sr(S, kind, seed * 0x9E3779B97F4A7C15 % 2 ** 64, 0)
        assert (e == 127).all() and np.array_equal(q, rne), (kind, seed)


@pytest.mark.parametrize("kind", SR.KINDS)
def test_expectation_is_within_2_to_the_minus_17_of_a_step(kind):
    """Over all 65,536 values of r: P(up) = round(T) / 65536 (a T that ends in .5 counts down: r + 0.5 < T is strict), so
    E[result] - |y| is at most 2^-17 of hi - lo."""
    G = SR.grid(kind)
    rng = np.random.default_rng(3)
    i = rng.integers(0, G.size - 1, 200)
    y = (G[i] + (G[i + 1] - G[i]) * rng.random(200)).astype(np.float32)
    y = np.concatenate([y, ((G[:-1] + G[1:]) / 2).astype(np.float32)])
    idx, exact, T = SR.neighbours(y, kind)
    r = np.arange(65536)
    worst = 0.0
    for k in range(y.size):
        ups = int((~exact[k] & (r + 0.5 < T[k])).sum())
        assert ups == max(int(np.ceil(T[k] - 0.5)), 0), (kind, float(y[k]))
        worst = max(worst, abs(ups / 65536 - T[k] / 65536))
    assert worst <= 2.0 ** -17, worst


def host(kind, S, seed, first):
    raw, sc = fmi_amd.mx_quantize_sr_host(SR.DTYPE_ID[kind], S, seed, first)
    assert raw.size == ((S.size + 1) // 2 if kind == "e2m1" else S.size) and sc.size == MX.blocks(S.size)
    if kind == "e2m1" and S.size % 2:
        assert raw[-1] >> 4 == 0
    return SR.codes_of(raw, kind, S.size), sc


def host_inputs(kind, n):
    """Sums of the visible family, with a NaN block, an inf block and an all-zero block where the bucket has room."""
    xs, es = SR.visible_inputs(kind, 1000, 8)
    S = SR.values("allreduce", kind, xs, es)[:n].copy()
    if n >= 1000:
        S[100] = np.nan
        S[5 * 32 + 31] = -np.inf
        S[7 * 32:8 * 32] = 0
        S[9 * 32:10 * 32] = np.float32(-0.0)
        S[11 * 32 + 3] = np.float32(1e-42)  # an f32 subnormal beside ordinary values
    return S


@pytest.mark.parametrize("kind", SR.KINDS)
def test_host_call_equals_the_definition(kind):
    for n in (0, 1, 2, 31, 32, 33, 63, 64, 65, 1000):
        S = host_inputs(kind, n)
        rne, rne_sc = SR.quant_rne(S, kind) if n else (np.empty(0, np.uint8), np.empty(0, np.uint8))
        for first in SR.FIRSTS:
            for seed in SR.SEEDS:
                want, want_sc = SR.quant_sr(S, kind, seed, first)
                got, got_sc = host(kind, S, seed, first)
                assert np.array_equal(got_sc, want_sc) and np.array_equal(got_sc, rne_sc), (kind, n, first, seed)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (kind, n, first, seed, bad[:8], got[bad[:8]], want[bad[:8]])
        if n == 1000:
            assert (want_sc[[3, 5]] == 255).all() and (want[3 * 32:4 * 32] == (0 if kind == "e2m1" else 0x7F)).all()
            assert (want[7 * 32:8 * 32] == 0).all() and (want[9 * 32:10 * 32] == SR.FORMAT[kind][2]).all()


@pytest.mark.parametrize("kind", SR.KINDS)
def test_host_call_at_chosen_r(kind):
    """The C++ rounding at r = 0, 1, 32767, 32768, 65534, 65535: the stream positions of seed 0 whose r is one of them
    hold, in blocks pinned at scale 2^0, values whose T lies at and next to r + 0.5."""
    n = 1 << 21
    r = SR.rbits(np.arange(n, dtype=np.uint64), 0)
    G = SR.grid(kind)
    S = np.zeros(n, np.float32)
    S[0::32] = SR.max_finite(kind)
    rng = np.random.default_rng(4)
    for edge in R_EDGES:
        at = np.flatnonzero((r == edge) & (np.arange(n) % 32 != 0))
        assert at.size >= 8, (edge, at.size)
        i = rng.integers(0, G.size - 1, at.size)
        t = G[i] + (G[i + 1] - G[i]) * (2 * edge + 1) / 131072  # T == r + 0.5 exactly, where f32 holds it
        v = t.astype(np.float32)
        v = np.where(np.arange(at.size) % 3 == 1, np.nextafter(v, np.float32(np.inf)), np.where(np.arange(at.size) % 3 == 2, np.nextafter(v, np.float32(0)), v))
        S[at] = np.minimum(v, SR.max_finite(kind)) * np.where(np.arange(at.size) % 2, -1, 1).astype(np.float32)
    want, want_sc = SR.quant_sr(S, kind, 0, 0)
    got, got_sc = host(kind, S, 0, 0)
    assert (want_sc == 127).all() and np.array_equal(got_sc, want_sc) and np.array_equal(got, want)


@pytest.mark.parametrize("kind", SR.KINDS)
def test_a_bucket_quantized_in_two_calls_equals_one_call(kind):
    S = host_inputs(kind, 1000)
    whole, whole_sc = host(kind, S, SR.SEEDS[2], 64)
    for split in (32, 960):
        a, a_sc = host(kind, S[:split], SR.SEEDS[2], 64)
        b, b_sc = host(kind, S[split:], SR.SEEDS[2], 64 + split)
        assert np.array_equal(np.concatenate([a, b]), whole) and np.array_equal(np.concatenate([a_sc, b_sc]), whole_sc), (kind, split)


@pytest.mark.parametrize("kind", SR.KINDS)
def test_the_visible_family_shows_the_rounding(kind):
    """P = 8, scale bytes 126..128, random codes: on the definition alone, SR differs from round-to-nearest, and two seeds
    from each other, on at least 5 % of the elements. tests/test_gpu_mx_sr.py runs this family."""
    xs, es = SR.visible_inputs(kind, M4.N_TILE, 8)
    S = SR.values("allreduce", kind, xs, es)
    rne, rne_sc = SR.quant_rne(S, kind)
    a, a_sc = SR.quant_sr(S, kind, SR.SEEDS[1], 32)
    b, _ = SR.quant_sr(S, kind, SR.SEEDS[2], 32)
    c, _ = SR.quant_sr(S, kind, SR.SEEDS[1], 64)
    assert np.array_equal(a_sc, rne_sc) and (rne_sc != 255).all()
    assert (a != rne).mean() >= 0.05 and (a != b).mean() >= 0.05 and (a != c).mean() >= 0.05, ((a != rne).mean(), (a != b).mean())
    # a shorter bucket is a prefix of a longer one
    ys, fs = SR.visible_inputs(kind, 100, 8)
    assert all(np.array_equal(y, x[:100]) for x, y in zip(xs, ys)) and all(np.array_equal(f, e[:4]) for e, f in zip(es, fs))


# ---- the host-side checks -----------------------------------------------------------------------------------------------
def test_host_call_rejections():
    lib = _lib.load()
    src = np.ones(64, np.float32)
    out, sc = np.zeros(64, np.uint8), np.zeros(2, np.uint8)
    fp = src.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    call = lambda dtype, n, seed, first, o=out.ctypes.data, s=sc.ctypes.data, p=fp: lib.fmi_host_mx_quantize_sr(dtype, o, s, p, n, seed, first)  # noqa: E731
    assert call(12, 64, 1, 0) == 0 and call(15, 0, 1, 0, None, None, None) == 0  # n = 0 succeeds
    assert call(12, 64, 1, 16) == _lib.FMI_ERR_INVALID and "multiple of 32" in _lib.last_error()
    assert call(12, 64, 1, 2 ** 64 - 32) == _lib.FMI_ERR_INVALID and "wraps" in _lib.last_error()
    assert call(12, 32, 1, 2 ** 64 - 32) == _lib.FMI_ERR_INVALID  # first + n = 2^64 wraps as well
    assert call(12, 31, 1, 2 ** 64 - 32) == 0
    assert call(1, 64, 1, 0) == _lib.FMI_ERR_INVALID and "MX bucket" in _lib.last_error()
    assert call(12, 64, 1, 0, None) == _lib.FMI_ERR_INVALID and "null buffer" in _lib.last_error()
    with pytest.raises(ValueError):
        fmi_amd.mx_quantize_sr_host(fmi_amd.DType.F32, src, 1)
    with pytest.raises(ValueError):
        fmi_amd.mx_quantize_sr_host(fmi_amd.DType.F4E2M1, src, -1)


def test_device_calls_reject_on_the_host_without_a_device():
    """seed == NULL or misaligned, first % 32 != 0 and a wrapping first + n are FMI_ERR_INVALID before a device is needed, as is what
    the round-to-nearest calls refuse."""
    lib = _lib.load()
    word = ctypes.c_uint64(1)
    seed = ctypes.cast(ctypes.pointer(word), ctypes.c_void_p)
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    one = (ctypes.c_void_p * 2)(p, p)
    INV = _lib.FMI_ERR_INVALID

    def tree(op=0, dtype=15, alg=0, seed=seed, first=0, n=64, P=2, out_scales=p):
        return lib.fmi_dev_reduce_tree_mx_sr(op, dtype, alg, p, out_scales, one, one, seed, first, P, 0, n, None)

    def quant(dtype=15, src_dtype=0, seed=seed, first=0, n=64):
        return lib.fmi_dev_mx_quantize_sr(dtype, p, p, src_dtype, p, n, seed, first, None)

    def comm(op=0, dtype=15, alg=0, seed=seed, first=0, n=64):
        return lib.fmi_comm_allreduce_mx_sr(None, op, dtype, alg, p, p, p, p, n, seed, first, None)

    for call in (tree, quant, comm):
        assert call(seed=None) == INV and "seed is NULL" in _lib.last_error(), call.__name__
        assert call(seed=ctypes.c_void_p(seed.value + 4)) == INV and "8-byte aligned" in _lib.last_error(), call.__name__
        assert call(first=48) == INV and "multiple of 32" in _lib.last_error(), call.__name__
        assert call(first=2 ** 64 - 64, n=65) == INV and "wraps" in _lib.last_error(), call.__name__
        assert call(dtype=0) == INV and "MX bucket" in _lib.last_error(), call.__name__
    assert tree(op=2) == INV and "FMI_OP_SUM" in _lib.last_error()
    assert tree(alg=3) == INV and "scan" in _lib.last_error()
    assert tree(out_scales=None) == INV and "out_scales is NULL" in _lib.last_error()
    assert tree(P=0) == INV
    assert quant(src_dtype=12) == INV and "src_dtype" in _lib.last_error()
    assert comm(op=3) == INV and comm(alg=1) == INV and "ALLREDUCE or REDUCE_LTR" in _lib.last_error()
    assert quant(n=0) == 0
    c = ctypes.c_int(-1)
    lib.fmi_dev_count(ctypes.byref(c))
    if c.value == 0:  # valid arguments reach the device check, not a kernel
        assert tree() == _lib.FMI_ERR_NO_DEVICE and quant() == _lib.FMI_ERR_NO_DEVICE
