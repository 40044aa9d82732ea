"""MXFP4 (FMI_F4E2M1 in the MX calls) without a GPU: the tests' own definition (tests/_mxfp4.py) against a brute-force
f64 rounding, what the scale rule at EMAX = 2 guarantees, the order cases the GPU test relies on, the host-side
validation through the C-ABI, and the Python layer's byte counts and refusals."""
import ctypes

import numpy as np
import pytest

from fmi_amd import _lib
from tests import _fp8 as F
from tests import _mx as MX
from tests import _mxfp4 as M

F4 = 15


def _brute_narrow(y):
    """Nearest of the eight magnitudes in f64 (exact: the distances are differences of f32 values), ties to the even code."""
    y = np.asarray(y, np.float32)
    a = np.abs(y.astype(np.float64))
    d = np.abs(a[:, None] - M.MAGNITUDES.astype(np.float64)[None, :])
    best = d.min(axis=1)
    code = np.zeros(a.size, np.int64)
    for c in range(7, -1, -1):  # the lowest code first among equals ...
        code = np.where(d[:, c] == best, c, code)
    up = code + 1
    tie = (up <= 7) & (d[np.arange(a.size), np.minimum(up, 7)] == best)
    code = np.where(tie & (code % 2 == 1), up, code)  # ... and the even one of a tie
    return (code | (np.signbit(y).astype(np.int64) << 3)).astype(np.uint8)


def test_narrow_is_nearest_with_ties_to_the_even_code():
    b = F.boundary_f32()
    b = b[np.isfinite(b) & (np.abs(b) <= 6)]
    assert b.size > 190000, b.size
    assert np.array_equal(M.narrow(b), _brute_narrow(b))
    for v, c in M.TIES:
        assert M.narrow(np.float32([v]))[0] == c and M.narrow(np.float32([-v]))[0] == (c | 8), v
        lo, hi = np.nextafter(np.float32(v), np.float32(0)), np.nextafter(np.float32(v), np.float32(8))
        assert M.narrow(np.float32([lo]))[0] in (c, c - 1) and M.narrow(np.float32([hi]))[0] in (c, c + 1)
        assert M.narrow(np.float32([lo]))[0] != M.narrow(np.float32([hi]))[0]
    assert M.narrow(np.float32([0.0]))[0] == 0 and M.narrow(np.float32([-0.0]))[0] == 8
    assert M.narrow(np.float32([-0.2]))[0] == 8
    assert M.narrow(np.float32([2.0 ** -149, -(2.0 ** -149), 6.0, -6.0])).tolist() == [0, 8, 7, 15]


def test_widen_of_narrow_is_the_identity_on_the_16_codes():
    codes = np.arange(16, dtype=np.uint8)
    assert np.array_equal(M.narrow(M.widen(codes)), codes)
    assert M.widen(codes)[:8].tolist() == [0, 0.5, 1, 1.5, 2, 3, 4, 6]
    assert np.signbit(M.widen(codes)[8:]).all()
    assert np.array_equal(M.unpack(M.pack(codes[:15]), 15), codes[:15]) and M.pack(codes[:15])[-1] == 0x0E


def test_dequant_is_one_multiply_with_the_special_scales():
    codes = np.repeat(np.arange(16, dtype=np.uint8), 2)  # one block, every code twice
    for e in range(255):
        got = M.dequant(codes, np.array([e], np.uint8))
        exact = M.widen(codes).astype(np.float64) * 2.0 ** (e - 127)
        ok = np.abs(exact) <= np.finfo(np.float32).max
        assert np.array_equal(got[ok].astype(np.float64), exact[ok]) and np.array_equal(np.signbit(got), np.signbit(exact)), e
        assert np.isinf(got[~ok]).all()
    assert np.isnan(M.dequant(codes, np.array([255], np.uint8))).all()          # zeros included
    assert M.dequant(codes, np.array([0], np.uint8))[2] == np.float32(2.0 ** -128)  # 0.5 * 2^-127: a subnormal
    assert np.isinf(M.dequant(codes, np.array([254], np.uint8))[8])             # 2 * 2^127


def test_quant_of_dequant_keeps_the_bytes_of_top_binade_blocks():
    rng = np.random.default_rng(5)
    nb = 4096
    q = rng.integers(0, 16, nb * 32).astype(np.uint8)
    e = rng.integers(3, 250, nb).astype(np.uint8)
    big = np.abs(M.widen(q)).reshape(nb, 32).max(axis=1)
    top = big >= 4  # the top binade [2^EMAX, 6]
    assert top.sum() > nb // 2
    q2, e2 = M.quant(M.dequant(q, e))
    assert np.array_equal(e2[top], e[top])
    rows = np.repeat(top, 32)
    assert np.array_equal(q2[rows], q[rows])


def test_no_element_of_a_finite_block_exceeds_6():
    rng = np.random.default_rng(11)
    nb = 20000
    top = rng.integers(0, 255, nb)[:, None]
    exp = np.clip(top - rng.integers(0, 6, (nb, 32)), 0, 254).astype(np.uint32)
    bits = (exp << np.uint32(23)) | rng.integers(0, 1 << 23, (nb, 32)).astype(np.uint32)
    bits |= rng.integers(0, 2, (nb, 32)).astype(np.uint32) << np.uint32(31)
    # some blocks' largest element on, just below and just above the threshold mantissa 0x400000
    edge = rng.integers(0, 3, nb).astype(np.uint32)
    bits[:, 0] = np.where(rng.integers(0, 4, nb) == 0, (top[:, 0].astype(np.uint32) << np.uint32(23)) | (np.uint32(0x3FFFFF) + edge), bits[:, 0])
    S = bits.reshape(-1).view(np.float32)
    # the extremes: a block of FLT_MAX, of the smallest subnormal, of 6 * 2^125, of zeros
    fmax = np.finfo(np.float32).max
    ext = np.concatenate([np.full(32, fmax), np.full(32, 2.0 ** -149), np.full(32, -fmax), np.zeros(32)]).astype(np.float32)
    S = np.concatenate([ext, S])
    y, ee, e = M.scaled(S)
    assert (e != 255).all() and e.max() <= 253
    assert (np.abs(y) <= 6).all() and np.isfinite(y).all()
    assert e[0] == 253 and (M.quant(S)[0][:32] == 6).all()       # FLT_MAX: e_out 253, element 4 (code 6)
    assert e[1] == 0 and e[3] == 0
    # the smallest such scale: a block with e_out > 0 has an element above half the maximum
    q, _ = M.quant(S)
    big = np.abs(M.widen(q)).reshape(-1, 32).max(axis=1)
    assert (big[e > 0] >= 3).all()


def test_a_nan_block_stores_zeros_and_byte_255():
    S = np.linspace(-5, 5, 128).astype(np.float32)
    S[5], S[3 * 32 + 31] = np.inf, np.nan
    q, e = M.quant(S)
    assert e.tolist()[0] == 255 and e[3] == 255 and (q[:32] == 0).all() and (q[96:] == 0).all()
    q0, e0 = M.quant(np.linspace(-5, 5, 128).astype(np.float32))
    assert np.array_equal(e[[1, 2]], e0[[1, 2]]) and np.array_equal(q[32:96], q0[32:96])
    assert np.isnan(M.dequant(q, e)[:32]).all()


def _share(a, b):
    return float((a.view(np.uint32) != b.view(np.uint32)).mean())


@pytest.mark.parametrize("P", M.ORDER_PEERS)
def test_the_order_cases_show_the_bracketing(P):
    """On the inputs tests/test_gpu_mxfp4.py uses (M.order_inputs(P, N_FUSED) and its cuts to N_TILE and 33, which are
    M.order_inputs at those lengths: scale bytes 112..142, f32 output) the three programs differ pairwise in at least 2 %
    of the elements, so a kernel that ran the wrong program could not pass all three. Measured with this generator, in %
    of elements, allreduce against reduce_ltr / allreduce against reduce at root P - 1 / reduce_ltr against that reduce:
        n = 8305:   P = 3  0.48 / 0 / 0.48    P = 8  5.31 / 6.31 / 7.41    P = 13  15.95 / 16.11 / 14.27    P = 16  17.90 / 14.21 / 18.87
        n = 12295:  P = 3  0.46 / 0 / 0.46    P = 8  5.49 / 6.47 / 7.43    P = 13  14.74 / 15.17 / 13.17    P = 16  17.78 / 13.95 / 18.87
    (At P = 3 allreduce and reduce at root 2 are the same bracketing.) With 120..134 every partial sum is exact and the
    share is 0 at every P; the E2M1 output hides the order too, which is why it pins the amax, the scale byte and the
    narrowing instead."""
    from tests.test_gpu_fp8_scaled import N_FUSED

    long_xs, long_es = M.order_inputs(P, N_FUSED)
    for n in (M.N_TILE, N_FUSED):
        xs, es = M.order_inputs(P, n)
        # the GPU test's cut of the long bucket IS this bucket
        assert all(np.array_equal(x, lx[:n]) for x, lx in zip(xs, long_xs))
        assert all(np.array_equal(e, le[:MX.blocks(n)]) for e, le in zip(es, long_es))
        a, _ = M.expected("allreduce", xs, es, "sum", "f32")
        b, _ = M.expected("reduce_ltr", xs, es, "sum", "f32")
        c, _ = M.expected("reduce", xs, es, "sum", "f32", root=P - 1)
        shares = {"allreduce / reduce_ltr": _share(a, b), "allreduce / reduce at root P - 1": _share(a, c),
                  "reduce_ltr / reduce at root P - 1": _share(b, c)}
        for pair, share in shares.items():
            print(f"P = {P}, n = {n}: {pair} differ in {100 * share:.2f} % of the elements")
            assert share >= 0.02, (P, n, pair, share)
    xs, es = M.random_inputs(M.N_TILE, P, 1000 + P, 120, 134)
    a, _ = M.expected("allreduce", xs, es, "sum", "f32")
    b, _ = M.expected("reduce_ltr", xs, es, "sum", "f32")
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_a_shorter_bucket_is_a_prefix_of_a_longer_one():
    """What lets the GPU test cut one long draw to every size: per-peer streams."""
    long_xs, long_es = M.random_inputs(5000, 4, 77, 100, 150)
    for n in (1, 33, 4097):
        xs, es = M.random_inputs(n, 4, 77, 100, 150)
        assert all(np.array_equal(x, lx[:n]) for x, lx in zip(xs, long_xs))
        assert all(np.array_equal(e, le[:MX.blocks(n)]) for e, le in zip(es, long_es))
    assert not np.array_equal(long_xs[0], long_xs[1]) and not np.array_equal(long_es[0], long_es[1])
    assert set(np.concatenate(long_xs).tolist()) == set(range(16))


# ---------------------------------------------------------------------------------------------------------------------
# the C-ABI's host-side checks: no device is needed (refusals come first; the valid calls are of zero elements)
# ---------------------------------------------------------------------------------------------------------------------
def _bufs():
    b = [ctypes.create_string_buffer(256) for _ in range(4)]
    p = [ctypes.addressof(x) for x in b]
    return b, p, (ctypes.c_void_p * 2)(p[0], p[1]), (ctypes.c_void_p * 2)(p[2], p[3])


def _past_the_checks(rc):
    c = ctypes.c_int(-1)
    _lib.load().fmi_dev_count(ctypes.byref(c))
    return rc == _lib.FMI_ERR_NO_DEVICE if c.value <= 0 else rc in (_lib.FMI_ERR_NO_DEVICE, 0)


@pytest.mark.parametrize("dtype", [F4, F4 | 0x100])
def test_the_mx_calls_accept_dtype_15(dtype):
    """Zero elements: nothing is launched on these host pointers. On the parent commit every one of these answered
    "dtype 15 is not FMI_F8E4M3 or FMI_F8E5M2"."""
    from fmi_amd.comm import Comm, Transport, unique_id

    lib = _lib.load()
    keep, p, ins, scs = _bufs()
    for out_dtype, osc in ((F4, p[3]), (0, None)):
        for op in (0, 5):
            for alg in (0, 1, 2):
                rc = lib.fmi_dev_reduce_tree_mx(op, dtype, alg, out_dtype, p[2], osc, ins, scs, 2, 0, 0, None)
                assert _past_the_checks(rc), (op, alg, out_dtype, rc, _lib.last_error())
    for wide in (0, 10, 11):
        assert lib.fmi_dev_mx_quantize(F4, p[0], p[1], wide, p[2], 0, None) == 0, _lib.last_error()
        assert lib.fmi_dev_mx_dequantize(wide, p[0], F4, p[1], p[2], 0, None) == 0, _lib.last_error()
    c0 = Comm(unique_id(Transport.LOCAL), 1, 0)
    h = ctypes.c_void_p(c0.handle)
    for out_dtype, osc in ((F4, p[3]), (0, None)):
        rc = lib.fmi_comm_allreduce_mx(h, 0, dtype, 0, out_dtype, p[0], p[1], p[2], osc, 0, None)
        assert _past_the_checks(rc), (out_dtype, rc, _lib.last_error())
    c0.destroy()


def test_the_mx_calls_still_check_the_rest_at_dtype_15():
    lib = _lib.load()
    keep, p, ins, scs = _bufs()
    for args, reason in (((1, F4, 0, F4), "op 1 is not valid here"), ((0, F4, 3, F4), "scan algorithm"), ((0, F4, 0, 12), "out_dtype 12"),
                         ((0, 12, 0, F4), "out_dtype 15"), ((0, F4, 0, 11), "out_dtype 11")):
        assert lib.fmi_dev_reduce_tree_mx(*args, p[2], p[3], ins, scs, 2, 0, 64, None) == _lib.FMI_ERR_INVALID, args
        assert reason in _lib.last_error(), (args, _lib.last_error())
    assert lib.fmi_dev_reduce_tree_mx(0, F4, 0, F4, p[2], None, ins, scs, 2, 0, 64, None) == _lib.FMI_ERR_INVALID
    assert "out_scales is NULL" in _lib.last_error()
    assert lib.fmi_dev_mx_quantize(F4, p[0], p[1], 1, p[2], 32, None) == _lib.FMI_ERR_INVALID
    assert "src_dtype 1 must be FMI_F32, FMI_F16 or FMI_BF16" in _lib.last_error()
    assert lib.fmi_dev_mx_dequantize(F4, p[0], F4, p[1], p[2], 32, None) == _lib.FMI_ERR_INVALID
    assert "dst_dtype 15 must be FMI_F32, FMI_F16 or FMI_BF16" in _lib.last_error()
    # the existing refusals still name the two 8-bit floats, and now the third element type after them
    for dt in (7, 2, 14):
        assert lib.fmi_dev_reduce_tree_mx(0, dt, 0, dt, p[2], p[3], ins, scs, 2, 0, 64, None) == _lib.FMI_ERR_INVALID
        msg = _lib.last_error()
        assert f"dtype {dt} is not FMI_F8E4M3 or FMI_F8E5M2" in msg and "FMI_F4E2M1" in msg, msg
        assert lib.fmi_dev_mx_quantize(dt, p[0], p[1], 0, p[2], 32, None) == _lib.FMI_ERR_INVALID
        assert f"dtype {dt} is not FMI_F8E4M3 or FMI_F8E5M2" in _lib.last_error()


@pytest.mark.parametrize("dtype", [F4, F4 | 0x100])
def test_every_other_entry_point_refuses_dtype_15_on_the_host(dtype):
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
    for name, call in calls.items():
        rc = call()
        msg = _lib.last_error()
        assert rc == _lib.FMI_ERR_INVALID, (name, rc, msg)
        assert "FMI_F4E2M1" in msg and f"dtype {D}" in msg, (name, msg)
    c0.destroy()
    assert lib.fmi_abi_version() == 1


# ---------------------------------------------------------------------------------------------------------------------
# the Python layer: buckets over raw pointers that are never dereferenced
# ---------------------------------------------------------------------------------------------------------------------
def test_bucket_byte_counts_and_views():
    import fmi_amd
    from fmi_amd import Bucket, DType

    assert int(DType.F4E2M1) == 15
    for n, nbytes in ((0, 0), (1, 1), (2, 1), (31, 16), (32, 16), (33, 17), (8305, 4153)):
        b = Bucket(n, DType.F4E2M1, ptr=4096)
        assert b.n == n and b.nbytes == nbytes, (n, b.nbytes)
    b = Bucket(70, DType.F4E2M1, ptr=4096)
    v = b.view(6, 33)
    assert v.ptr == 4096 + 3 and v.n == 33 and v.nbytes == 17
    with pytest.raises(ValueError, match="even element offset"):
        b.view(3, 8)
    with pytest.raises(ValueError, match="out of range"):
        b.view(40, 32)
    with pytest.raises(ValueError, match="size mismatch"):
        b.upload(np.zeros(70, np.uint8))  # 35 packed bytes, not 70
    codes = np.arange(16, dtype=np.uint8)[:15]
    packed = fmi_amd.fp4_pack(codes)
    assert packed.size == 8 and packed[0] == 0x10 and packed[-1] == 0x0E
    assert np.array_equal(fmi_amd.fp4_unpack(packed, 15), codes)
    assert np.array_equal(packed, M.pack(codes))
    with pytest.raises(ValueError):
        fmi_amd.fp4_unpack(packed, 17)
    with pytest.raises(ValueError):
        fmi_amd.fp4_pack([16])


def test_python_refuses_f4e2m1_outside_the_mx_calls():
    import fmi_amd
    from fmi_amd import Alg, Bucket, DType, Op
    from fmi_amd.comm import Comm, Transport, unique_id

    def bk(n, dt=DType.F4E2M1):
        return Bucket(n, dt, ptr=4096)

    n = 64
    a, b, c = bk(n), bk(n), bk(n)
    refused = (
        lambda: fmi_amd.reduce_pair(Op.SUM, a, b),
        lambda: fmi_amd.reduce_pair_batch(Op.SUM, [(a, b)]),
        lambda: fmi_amd.combine(Op.SUM, c, a, b),
        lambda: fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, c, [a, b]),
        lambda: fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, c, [a, b], accumulate_f32=True),
        lambda: fmi_amd.reduce_tree_scaled(Alg.ALLREDUCE, c, [a, b], bk(2, DType.F32)),
        lambda: fmi_amd.scan_peers(Op.SUM, Alg.SCAN, [a, b], [a, b]),
        lambda: fmi_amd.mean_scale(a, 2),
        lambda: fmi_amd.convert(bk(n, DType.F32), a),
        lambda: fmi_amd.convert(a, bk(n, DType.F32)),
        lambda: a.fill_synthetic(1, 0),
        lambda: fmi_amd.host_reduce_pair(Op.SUM, np.zeros(8, np.uint8), np.zeros(8, np.uint8), dtype=DType.F4E2M1),
    )
    for i, call in enumerate(refused):
        with pytest.raises(ValueError, match="F4E2M1|F8E4M3 or F8E5M2"):
            call()
    c0 = Comm(unique_id(Transport.LOCAL), 1, 0)
    for call in (lambda: c0.allreduce(Op.SUM, a, b), lambda: c0.reduce(Op.SUM, a, b, 0), lambda: c0.scan(Op.SUM, a, b),
                 lambda: c0.allreduce_scaled(a, bk(1, DType.F32), b),
                 lambda: c0.allreduce_host(Op.SUM, np.zeros(8, np.uint8), np.zeros(8, np.uint8), dtype=DType.F4E2M1)):
        with pytest.raises(ValueError, match="F4E2M1|F8E4M3 or F8E5M2"):
            call()
    c0.destroy()
    # the MX calls' own checks hold for it: lengths in ELEMENTS, scale bytes per 32 elements
    sc = [bk(3, DType.F8E8M0) for _ in range(2)]
    ins = [bk(70), bk(70)]
    with pytest.raises(ValueError, match=r"ceil\(n / 32\) = 3 scale bytes for 70 elements, got 2"):
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, bk(70), bk(3, DType.F8E8M0), ins, [sc[0], bk(2, DType.F8E8M0)])
    with pytest.raises(ValueError, match="out_scales is missing"):
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, bk(70), None, ins, sc)
    with pytest.raises(ValueError, match="in their dtype or in F32"):
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, bk(70, DType.F8E4M3), bk(3, DType.F8E8M0), ins, sc)
    with pytest.raises(ValueError, match="needs F8E4M3 or F8E5M2 input buckets, got F32"):
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, bk(70, DType.F32), None, [bk(70, DType.F32)] * 2, sc)
