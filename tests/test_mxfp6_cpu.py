"""MXFP6 without a GPU: the numpy definition (tests/_mxfp6.py) against the closed forms, the packing, the ties, the scale
rule at its thresholds, the host stochastic-rounding call at FMI_F6E2M3 / FMI_F6E3M2, every refusal, the Python layer's
byte counts, and the order condition the GPU test relies on."""
import ctypes

import numpy as np
import pytest

from fmi_amd import _lib
from tests import _mx as MX
from tests import _mx_sr as SR
from tests import _mxfp6 as M

KINDS = M.KINDS
ID = M.DTYPE_ID


# ---- the tables ---------------------------------------------------------------------------------------------------------
def test_tables_against_the_closed_forms():
    e2m3 = [m / 8 for m in range(8)] + [(1 + m / 8) * 2.0 ** (e - 1) for e in (1, 2, 3) for m in range(8)]
    e3m2 = [m / 16 for m in range(4)] + [(1 + m / 4) * 2.0 ** (e - 3) for e in range(1, 8) for m in range(4)]
    for kind, want in (("e2m3", e2m3), ("e3m2", e3m2)):
        assert M.MAGNITUDES[kind].tolist() == want
        assert (np.diff(M.MAGNITUDES[kind]) > 0).all(), "magnitude codes ascend in value"
        t = M.widen(np.arange(64), kind)
        assert np.array_equal(t[:32], M.MAGNITUDES[kind]) and np.array_equal(t[32:], -M.MAGNITUDES[kind])
        assert np.signbit(t[32]) and t[32] == 0, "code 0x20 is -0"
        assert np.array_equal(M.narrow(t, kind), np.arange(64)), "every grid value narrows to its own code"
    assert M.MAX["e2m3"] == 7.5 and M.MAX["e3m2"] == 28.0


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 6, 7, 8, 31, 32, 33, 8305])
def test_pack_unpack_round_trip(n):
    import fmi_amd

    codes = np.random.default_rng(n).integers(0, 64, n).astype(np.uint8)
    p = M.pack(codes)
    assert p.size == (3 * n + 3) // 4 == M.nbytes(n)
    assert np.array_equal(M.unpack(p, n), codes)
    # the bit string by hand: bit j of the string is bit j % 8 of byte j // 8
    for i in range(min(n, 9)):
        got = sum(((int(p[(6 * i + k) // 8]) >> ((6 * i + k) % 8)) & 1) << k for k in range(6))
        assert got == codes[i]
    if n % 4:
        assert int(p[-1]) >> (6 * n % 8) == 0, "the last byte's unused high bits are 0"
    assert np.array_equal(fmi_amd.fp6_pack(codes), p)
    assert np.array_equal(fmi_amd.fp6_unpack(p, n), codes)


@pytest.mark.parametrize("kind", KINDS)
def test_all_31_ties_and_their_neighbours(kind):
    ts = M.ties(kind)
    assert len(ts) == 31
    for c, (v, code) in enumerate(ts):
        assert code % 2 == 0 and code in (c, c + 1)
        for s, bit in ((1, 0), (-1, 0x20)):
            w = np.float32(s * v)
            below, above = np.nextafter(w, np.float32(0)), np.nextafter(w, np.float32(s * 64))
            assert M.narrow([w], kind)[0] == code | bit
            assert M.narrow([below], kind)[0] == c | bit and M.narrow([above], kind)[0] == (c + 1) | bit


@pytest.mark.parametrize("kind", KINDS)
def test_scale_rule_at_the_thresholds(kind):
    _, _, _, emax, _ = M.FORMAT[kind]
    top = M.MAX[kind]
    for k in (-120, -3, 0, 5, 100):
        v = np.float32(top * 2.0 ** k)
        assert M.scale_bytes(np.array([v], np.float32), kind)[0] == 127 + k
        up = np.nextafter(v, np.float32(np.inf))
        assert M.scale_bytes(np.array([up], np.float32), kind)[0] == 127 + k + 1
        q, e = M.quant(np.array([v, up], np.float32)[:1], kind)
        assert q[0] == 31
    # the largest finite f32: e_out <= 253 (E2M3) / 251 (E3M2)
    big = np.array([np.finfo(np.float32).max], np.float32)
    assert M.scale_bytes(big, kind)[0] == 254 - emax + 1
    # clamped at 0: tiny and subnormal blocks
    for v in (2.0 ** -127, 2.0 ** -149, 0.0):
        assert M.scale_bytes(np.array([v], np.float32), kind)[0] == 0
    # NaN blocks: scale byte 255 and every code 0
    for bad in (np.inf, -np.inf, np.nan):
        S = np.array([1.0, bad] + [0.5] * 40, np.float32)
        q, e = M.quant(S, kind)
        assert e.tolist() == [255, M.scale_bytes(S[32:], kind)[0]] and (q[:32] == 0).all() and (q[32:] != 0).all()
    # no element of a finite block exceeds the largest element
    S = (np.random.default_rng(5).standard_normal(32 * 200) * 2.0 ** np.random.default_rng(6).integers(-30, 30, 32 * 200)).astype(np.float32)
    y, _, _ = M.scaled(S, kind)
    assert (np.abs(y) <= top).all()


@pytest.mark.parametrize("kind", KINDS)
def test_narrow_sr_forms_agree(kind):
    v = M.exhaustive_values(kind)
    rng = np.random.default_rng(11)
    y = np.concatenate([v, (rng.random(20000) * 2 - 1).astype(np.float32) * M.MAX[kind]]).astype(np.float32)
    for r in (np.zeros(y.size, np.int64), np.full(y.size, 65535), rng.integers(0, 65536, y.size)):
        a, b = M.narrow_sr(y, r, kind), M.narrow_sr_int(y, r, kind)
        assert np.array_equal(a, b)
    # a grid value never moves
    g = M.widen(np.arange(64), kind)
    assert np.array_equal(M.narrow_sr(g, np.full(64, 0), kind), np.arange(64))
    assert np.array_equal(M.narrow_sr(g, np.full(64, 65535), kind), np.arange(64))


# ---- the host call --------------------------------------------------------------------------------------------------------
def _host_sr(kind, S, seed, first):
    import fmi_amd

    raw, sc = fmi_amd.mx_quantize_sr_host(fmi_amd.DType(ID[kind]), S, seed, first)
    return raw, sc


@pytest.mark.parametrize("kind", KINDS)
def test_host_quantize_sr_equals_the_definition(kind):
    """Fails without the feature: "unknown dtype 16"."""
    rng = np.random.default_rng(3)
    S = (rng.standard_normal(32 * 40 + 19) * 2.0 ** rng.integers(-20, 20, 32 * 40 + 19)).astype(np.float32)
    S[64:96] = 0
    S[100] = np.inf
    S = np.concatenate([S, M.pinned_blocks(M.exhaustive_values(kind), kind)]).astype(np.float32)
    for n in (S.size, 1, 2, 3, 31, 33, 1299):
        for seed in SR.SEEDS:
            for first in SR.FIRSTS:
                raw, sc = _host_sr(kind, S[:n], seed, first)
                want, want_sc = M.quant_sr(S[:n], kind, seed, first)
                assert raw.size == M.nbytes(n)
                assert np.array_equal(sc, want_sc), (n, seed, first)
                assert np.array_equal(raw, M.pack(want)), (n, seed, first)
    # the scale bytes are the round-to-nearest rule's
    assert np.array_equal(_host_sr(kind, S, 1, 0)[1], M.quant(S, kind)[1])


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _bufs():
    b = [ctypes.create_string_buffer(256) for _ in range(4)]
    p = [ctypes.addressof(x) for x in b]
    return b, p, (ctypes.c_void_p * 2)(p[0], p[1]), (ctypes.c_void_p * 2)(p[2], p[3])


def _past_the_checks(rc):
    c = ctypes.c_int(-1)
    _lib.load().fmi_dev_count(ctypes.byref(c))
    return rc == _lib.FMI_ERR_NO_DEVICE if c.value <= 0 else rc in (_lib.FMI_ERR_NO_DEVICE, 0)


@pytest.mark.parametrize("dtype", [16, 17, 16 | 0x100, 17 | 0x100])
def test_the_mx_calls_accept_the_two_ids(dtype):
    from fmi_amd.comm import Comm, Transport, unique_id

    lib = _lib.load()
    keep, p, ins, scs = _bufs()
    st = dtype & 0xFF
    for out_dtype, osc in ((st, p[3]), (0, None)):
        for op in (0, 5):
            for alg in (0, 1, 2):
                rc = lib.fmi_dev_reduce_tree_mx(op, dtype, alg, out_dtype, p[2], osc, ins, scs, 2, 0, 0, None)
                assert _past_the_checks(rc), (op, alg, out_dtype, rc, _lib.last_error())
    for wide in (0, 10, 11):
        assert lib.fmi_dev_mx_quantize(st, p[0], p[1], wide, p[2], 0, None) == 0, _lib.last_error()
        assert lib.fmi_dev_mx_dequantize(wide, p[0], st, p[1], p[2], 0, None) == 0, _lib.last_error()
    c0 = Comm(unique_id(Transport.LOCAL), 1, 0)
    h = ctypes.c_void_p(c0.handle)
    for out_dtype, osc in ((st, p[3]), (0, None)):
        rc = lib.fmi_comm_allreduce_mx(h, 0, dtype, 0, out_dtype, p[0], p[1], p[2], osc, 0, None)
        assert _past_the_checks(rc), (out_dtype, rc, _lib.last_error())
    c0.destroy()


@pytest.mark.parametrize("st", [16, 17])
def test_the_mx_calls_still_check_the_rest(st):
    lib = _lib.load()
    keep, p, ins, scs = _bufs()
    other = 33 - st
    for args, reason in (((1, st, 0, st), "op 1 is not valid here"), ((0, st, 3, st), "scan algorithm"), ((0, st, 0, 12), "out_dtype 12"),
                         ((0, st, 0, other), f"out_dtype {other}"), ((0, 12, 0, st), f"out_dtype {st}")):
        assert lib.fmi_dev_reduce_tree_mx(*args, p[2], p[3], ins, scs, 2, 0, 64, None) == _lib.FMI_ERR_INVALID, args
        assert reason in _lib.last_error(), (args, _lib.last_error())
    assert lib.fmi_dev_reduce_tree_mx(0, st, 0, st, p[2], None, ins, scs, 2, 0, 64, None) == _lib.FMI_ERR_INVALID
    assert "out_scales is NULL" in _lib.last_error()
    assert lib.fmi_dev_mx_quantize(st, p[0], p[1], 1, p[2], 32, None) == _lib.FMI_ERR_INVALID
    assert "src_dtype 1 must be FMI_F32, FMI_F16 or FMI_BF16" in _lib.last_error()
    assert lib.fmi_dev_mx_dequantize(st, p[0], st, p[1], p[2], 32, None) == _lib.FMI_ERR_INVALID
    assert f"dst_dtype {st} must be FMI_F32, FMI_F16 or FMI_BF16" in _lib.last_error()
    seed = ctypes.c_uint64(1)
    assert lib.fmi_dev_reduce_tree_mx_sr(0, st, 0, p[2], p[3], ins, scs, ctypes.byref(seed), 16, 2, 0, 64, None) == _lib.FMI_ERR_INVALID
    assert "first 16 is not a multiple of 32" in _lib.last_error()
    # the refusal of a type that is no MX element names the new types after the old ones
    assert lib.fmi_dev_reduce_tree_mx(0, 7, 0, 7, p[2], p[3], ins, scs, 2, 0, 64, None) == _lib.FMI_ERR_INVALID
    msg = _lib.last_error()
    assert "dtype 7 is not FMI_F8E4M3 or FMI_F8E5M2" in msg and "FMI_F4E2M1" in msg and "FMI_F6E2M3" in msg and "FMI_F6E3M2" in msg


@pytest.mark.parametrize("dtype", [16, 17, 16 | 0x100, 17 | 0x100])
def test_every_other_entry_point_refuses_the_two_ids_on_the_host(dtype):
    from fmi_amd.comm import Comm, Transport, unique_id

    lib = _lib.load()
    keep, p, ins, outs = _bufs()
    f32p = ctypes.cast(p[3], ctypes.POINTER(ctypes.c_float))

    class Pair(ctypes.Structure):
        _fields_ = [("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("n", ctypes.c_size_t)]

    pd = (Pair * 1)(Pair(p[0], p[1], 8))
    c0 = Comm(unique_id(Transport.LOCAL), 1, 0)
    h = ctypes.c_void_p(c0.handle)
    D, st = dtype, dtype & 0xFF
    name = "FMI_F6E2M3" if st == 16 else "FMI_F6E3M2"
    calls = {
        "fmi_dev_reduce_pair": lambda: lib.fmi_dev_reduce_pair(0, D, p[0], p[1], 8, None),
        "fmi_dev_reduce_pair_batch": lambda: lib.fmi_dev_reduce_pair_batch(0, D, ctypes.cast(pd, ctypes.c_void_p), 1, None),
        "fmi_dev_combine": lambda: lib.fmi_dev_combine(0, D, p[0], p[1], p[2], 8, None),
        "fmi_dev_reduce_tree": lambda: lib.fmi_dev_reduce_tree(0, D, 0, p[2], ins, 2, 0, 8, None),
        "fmi_dev_reduce_tree avg": lambda: lib.fmi_dev_reduce_tree(5, D, 2, p[2], ins, 2, 0, 8, None),
        "fmi_dev_scan_peers": lambda: lib.fmi_dev_scan_peers(0, D, 3, outs, ins, 2, 8, None),
        "fmi_dev_mean_scale": lambda: lib.fmi_dev_mean_scale(D, p[0], 8, 2, None),
        "fmi_dev_convert dst": lambda: lib.fmi_dev_convert(D, p[0], 0, p[1], 8, None),
        "fmi_dev_convert src": lambda: lib.fmi_dev_convert(0, p[0], D, p[1], 8, None),
        "fmi_dev_reduce_tree_scaled": lambda: lib.fmi_dev_reduce_tree_scaled(0, D, 0, st, p[2], ins, f32p, None, None, 2, 0, 8, None),
        "fmi_dev_fill_synthetic": lambda: lib.fmi_dev_fill_synthetic(D, p[0], 8, 1, 0, None),
        "fmi_dev_fill_synthetic_at": lambda: lib.fmi_dev_fill_synthetic_at(D, p[0], 8, 1, 0, 0, None),
        "fmi_host_reduce_pair": lambda: lib.fmi_host_reduce_pair(0, D, p[0], p[1], 8),
        "fmi_comm_allreduce": lambda: lib.fmi_comm_allreduce(h, 0, D, 0, 0, p[0], p[1], 8, None),
        "fmi_comm_allreduce_scaled": lambda: lib.fmi_comm_allreduce_scaled(h, 0, D, 0, st, p[0], f32p, p[1], None, None, 8, None),
        "fmi_comm_allreduce_host": lambda: lib.fmi_comm_allreduce_host(h, 0, D, 0, 0, p[0], p[1], 8, 0),
        "fmi_comm_reduce": lambda: lib.fmi_comm_reduce(h, 0, D, 1, p[0], p[1], 8, 0, None),
        "fmi_comm_reduce_sendbuf": lambda: lib.fmi_comm_reduce_sendbuf(h, 0, D, 1, p[0], p[1], 8, 0, None),
        "fmi_comm_scan": lambda: lib.fmi_comm_scan(h, 0, D, 3, p[0], p[1], 8, None),
    }
    for what, call in calls.items():
        rc = call()
        msg = _lib.last_error()
        assert rc == _lib.FMI_ERR_INVALID, (what, rc, msg)
        assert name in msg and f"dtype {D}" in msg and "6-bit elements have no other kernel" in msg, (what, msg)
    c0.destroy()
    assert lib.fmi_abi_version() == 1


def test_the_refusal_of_dtype_15_keeps_its_words():
    lib = _lib.load()
    keep, p, ins, outs = _bufs()
    assert lib.fmi_dev_reduce_pair(0, 15, p[0], p[1], 8, None) == _lib.FMI_ERR_INVALID
    assert _lib.last_error().endswith("dtype 15 (FMI_F4E2M1) is valid only as the element type of the MX calls (fmi_dev_reduce_tree_mx, "
                                      "fmi_dev_mx_quantize, fmi_dev_mx_dequantize, fmi_comm_allreduce_mx): 4-bit elements have no other kernel")


# ---- the Python layer ---------------------------------------------------------------------------------------------------
def test_bucket_byte_counts_and_views():
    import fmi_amd
    from fmi_amd import Bucket, DType

    assert int(DType.F6E2M3) == 16 and int(DType.F6E3M2) == 17
    for dt in (DType.F6E2M3, DType.F6E3M2):
        for n, nb in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 3), (5, 4), (31, 24), (32, 24), (33, 25), (8305, 6229)):
            b = Bucket(n, dt, ptr=4096)
            assert b.n == n and b.nbytes == nb, (n, b.nbytes)
        b = Bucket(70, dt, ptr=4096)
        v = b.view(8, 33)
        assert v.ptr == 4096 + 6 and v.n == 33 and v.nbytes == 25
        for off in (1, 2, 3, 6):
            with pytest.raises(ValueError, match="multiple of 4"):
                b.view(off, 8)
        with pytest.raises(ValueError, match="out of range"):
            b.view(40, 32)
        with pytest.raises(ValueError, match="size mismatch"):
            b.upload(np.zeros(70, np.uint8))  # 53 packed bytes, not 70
    with pytest.raises(ValueError):
        fmi_amd.fp6_unpack(np.zeros(3, np.uint8), 5)
    with pytest.raises(ValueError):
        fmi_amd.fp6_pack([64])


def test_python_refuses_the_types_outside_the_mx_calls():
    import fmi_amd
    from fmi_amd import Alg, Bucket, DType, Op

    for dt in (DType.F6E2M3, DType.F6E3M2):
        a, b, c = (Bucket(64, dt, ptr=4096 + 64 * k) for k in range(3))
        for call in (lambda: fmi_amd.reduce_pair(Op.SUM, a, b), lambda: fmi_amd.combine(Op.SUM, c, a, b),
                     lambda: fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, c, [a, b]), lambda: fmi_amd.scan_peers(Op.SUM, Alg.SCAN, [a, b], [a, b]),
                     lambda: fmi_amd.mean_scale(a, 2), lambda: fmi_amd.convert(Bucket(64, DType.F32, ptr=8192), a),
                     lambda: a.fill_synthetic(1, 0)):
            with pytest.raises(ValueError, match=dt.name):
                call()
        with pytest.raises(ValueError, match=dt.name):
            fmi_amd.host_reduce_pair(Op.SUM, np.zeros(8, np.uint8), np.zeros(8, np.uint8), dtype=dt)
        # an MX call takes them, and checks the rest: a scale bucket of the wrong length
        sc = Bucket(1, DType.F8E8M0, ptr=4096)
        with pytest.raises(ValueError, match="scale bytes"):
            fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, c, sc, [a, b], [sc, sc])
        with pytest.raises(ValueError, match="their dtype or in F32"):
            fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, Bucket(64, DType.F4E2M1, ptr=4096), sc, [a, b], [sc, sc])


# ---- the order condition ------------------------------------------------------------------------------------------------
ROOTED = (("allreduce", lambda P: 0), ("reduce", lambda P: P - 1), ("reduce_ltr", lambda P: 0))


@pytest.mark.parametrize("P", M.ORDER_PEERS)
@pytest.mark.parametrize("kind", KINDS)
def test_order_condition(kind, P):
    """A cap, not a measurement: with scale bytes 112..142 each pair of bracketings differs in at least 4 % of the
    elements (half the smallest share measured: 7.8 %), all values finite; with 120..134 none differs."""
    for n in M.ORDER_SIZES:
        xs, es = M.order_inputs(P, n)
        S = {f: M.values(f, kind, xs, es, "sum", root(P)) for f, root in ROOTED}
        assert all(np.isfinite(v).all() for v in S.values())
        for a, b in (("allreduce", "reduce_ltr"), ("allreduce", "reduce"), ("reduce", "reduce_ltr")):
            share = np.mean(S[a].view(np.uint32) != S[b].view(np.uint32))
            print(f"{kind} P={P} n={n} {a}/{b}: {100 * share:.1f} %")
            assert share >= 0.04, (kind, P, n, a, b, share)
        xs, es = M.order_inputs(P, n, M.EXACT_RANGE)
        E = [M.values(f, kind, xs, es, "sum", root(P)) for f, root in ROOTED]
        assert np.array_equal(E[0].view(np.uint32), E[1].view(np.uint32)) and np.array_equal(E[0].view(np.uint32), E[2].view(np.uint32))


def test_a_shorter_bucket_is_a_prefix_of_a_longer_one():
    long_xs, long_es = M.random_inputs(5000, 4, 77, 100, 150)
    for n in (1, 33, 4097):
        xs, es = M.random_inputs(n, 4, 77, 100, 150)
        assert all(np.array_equal(x, lx[:n]) for x, lx in zip(xs, long_xs))
        assert all(np.array_equal(e, le[:MX.blocks(n)]) for e, le in zip(es, long_es))
    assert set(np.concatenate(long_xs).tolist()) == set(range(64))
