"""The MX (block-scaled FP8) calls without a GPU: the tests' own definition (tests/_mx.py) against torch's E8M0 and an
f64 evaluation, what the round-up scale rule guarantees, the four symbols, and the host-side validation."""
import ctypes
import os
import re

import numpy as np
import pytest

from fmi_amd import _lib
from tests import _fp8 as F
from tests import _mx as MX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fmi_dev_reduce_tree_mx", "fmi_dev_mx_quantize", "fmi_dev_mx_dequantize", "fmi_comm_allreduce_mx")


def test_scale32_is_torchs_e8m0():
    import torch

    e = np.arange(255, dtype=np.uint8)
    want = torch.from_numpy(e).view(torch.float8_e8m0fnu).to(torch.float32).numpy()
    assert np.array_equal(MX.scale32(e).view(np.uint32), want.view(np.uint32))
    assert MX.scale32(np.array([0], np.uint8))[0] == np.float32(2.0 ** -127)
    assert np.isnan(MX.scale32(np.array([255], np.uint8))[0])


@pytest.mark.parametrize("kind", F.KINDS)
def test_dequant_is_exact(kind):
    """widen(x) * scale32(e) is exact in f32 for every byte x scale pair that does not overflow: the f64 product (exact:
    4 significand bits times a power of two) rounds to itself."""
    q = np.repeat(np.arange(256, dtype=np.uint8), MX.BLOCK)          # one block per byte value
    w64 = F.widen(q, kind).astype(np.float64)
    pairs = 0
    for e in range(255):
        es = np.full(256, e, np.uint8)
        exact = w64 * np.float64(2.0) ** (e - 127)
        got = MX.dequant(q, es, kind)
        ok = np.isfinite(exact) & (np.abs(exact) <= np.finfo(np.float32).max)
        assert np.array_equal(got[ok].astype(np.float64), exact[ok]), (kind, e)
        assert np.array_equal(np.signbit(got[ok]), np.signbit(exact[ok])), (kind, e)
        pairs += int(ok[::MX.BLOCK].sum())
    assert pairs >= 240 * 255, pairs  # of 256 x 255: the NaN (and inf) bytes and the few products beyond f32 are left out
    # scale 255 makes every element NaN, a zero included
    assert np.isnan(MX.dequant(q, np.full(256, 255, np.uint8), kind)).all()


def _wide_range_blocks(kind, nblocks, seed):
    """Blocks whose magnitudes sit anywhere in the f32 exponent range: a per-block exponent from the whole range
    (subnormals included), elements within a few binades below it, random significands and signs."""
    rng = np.random.default_rng(seed)
    top = rng.integers(0, 255, nblocks)[:, None]
    exp = np.clip(top - rng.integers(0, 12, (nblocks, MX.BLOCK)), 0, 254).astype(np.uint32)
    bits = (exp << np.uint32(23)) | rng.integers(0, 1 << 23, (nblocks, MX.BLOCK)).astype(np.uint32)
    bits |= rng.integers(0, 2, (nblocks, MX.BLOCK)).astype(np.uint32) << np.uint32(31)
    # some blocks' largest element exactly on, just below and just above the threshold mantissa 0x600000
    edge = rng.integers(0, 3, nblocks).astype(np.uint32)
    bits[:, 0] = np.where(rng.integers(0, 4, nblocks) == 0, (top[:, 0].astype(np.uint32) << np.uint32(23)) | (np.uint32(0x5FFFFF) + edge),
                          bits[:, 0])
    return bits.reshape(-1).view(np.float32)


@pytest.mark.parametrize("kind", F.KINDS)
def test_round_up_rule_never_overflows_a_finite_block(kind):
    S = _wide_range_blocks(kind, 20000, 11)
    q, e = MX.quant(S, kind)
    assert (e != 255).all()
    assert e.max() <= (247 if kind == "e4m3" else 240), int(e.max())
    w = F.widen(q, kind)
    assert np.isfinite(w).all(), "a finite block produced an inf or a NaN element"
    # and the scale is the SMALLEST such power of two: a block with e_out > 0 has an element above half the maximum
    big = np.abs(w).reshape(-1, MX.BLOCK).max(axis=1)
    assert (big[e > 0] > F.MAX_FINITE[kind] / 2 * (1 - 2.0 ** -4)).all()
    # a block with an inf or a NaN is all NaN under scale 255
    S2 = S.copy()
    S2[5], S2[MX.BLOCK * 3 + 31] = np.inf, np.nan
    q2, e2 = MX.quant(S2, kind)
    assert e2[0] == 255 and e2[3] == 255 and (q2[:MX.BLOCK] == 0x7F).all() and (q2[3 * MX.BLOCK:4 * MX.BLOCK] == 0x7F).all()
    assert np.array_equal(e2[[1, 2]], e[[1, 2]])


@pytest.mark.parametrize("kind", F.KINDS)
def test_quant_of_dequant_is_the_identity_on_normal_blocks(kind):
    """The round trip. Where a block's largest element of q is normal in the 8-bit type, quant(dequant(q, e)) decodes
    to the same VALUES, bit for bit. It returns the same BYTES (q and e themselves) only where that element lies in the
    type's top binade, [2^EMAX, max]: the scale rule is canonical, so a block stored with headroom (largest element
    2^k, k < EMAX) comes back with scale e + k - EMAX (+ 1 above 1.75 * 2^k) and its elements moved up to match. Both
    are asserted; "the same bytes for every normal block" would contradict the rule for e_out."""
    rng = np.random.default_rng(3)
    ok = np.flatnonzero(np.isfinite(F.widen(np.arange(256, dtype=np.uint8), kind))).astype(np.uint8)
    nb = 4096
    q = ok[rng.integers(0, ok.size, nb * MX.BLOCK)]
    e = rng.integers(40, 215, nb).astype(np.uint8)
    v = MX.dequant(q, e, kind)
    q2, e2 = MX.quant(v, kind)
    v2 = MX.dequant(q2, e2, kind)
    big = np.abs(F.widen(q, kind)).reshape(nb, MX.BLOCK).max(axis=1)
    m = 3 if kind == "e4m3" else 2
    normal = big >= 2.0 ** (1 - (7 if kind == "e4m3" else 15))
    assert normal.sum() > nb // 2
    # values: always the same where the block's largest element is normal (rescaling by a power of two loses bits only
    # of elements that fall below the subnormal grid, which a smaller scale never causes)
    rows = np.repeat(normal, MX.BLOCK)
    assert np.array_equal(v2[rows].view(np.uint32), v[rows].view(np.uint32))
    # bytes: the same where the largest element sits in the type's top binade (then e_out is e itself)
    top = big >= 2.0 ** MX.EMAX[kind]
    assert top.sum() > 16 and m > 0
    assert np.array_equal(e2[top], e[top])
    assert np.array_equal(q2[np.repeat(top, MX.BLOCK)], q[np.repeat(top, MX.BLOCK)])


def test_helper_equals_a_hand_evaluation():
    """reduce_ltr at P = 3 over two blocks and a ragged third, every operation redone in f64 and rounded once."""
    kind, n = "e4m3", 70
    xs, es = MX.random_inputs(kind, n, 3, seed=9)
    v = [(F.widen(x, kind).astype(np.float64) * MX.scale32(MX.per_element(e, n)).astype(np.float64)).astype(np.float32) for x, e in zip(xs, es)]
    S = ((v[0].astype(np.float64) + v[1]).astype(np.float32).astype(np.float64) + v[2]).astype(np.float32)
    out, none = MX.expected_mx("reduce_ltr", kind, xs, es, "sum", "f32")
    assert none is None
    MX.assert_mx(out, None, S, None, kind, "f32", "S")
    avg, _ = MX.expected_mx("reduce_ltr", kind, xs, es, "avg", "f32")
    MX.assert_mx(avg, None, (S.astype(np.float64) * np.float64(np.float32(1) / np.float32(3))).astype(np.float32), None, kind, "f32", "mean")
    q, e = MX.expected_mx("reduce_ltr", kind, xs, es, "sum", "same")
    assert e.size == 3 and q.size == n
    for b in range(3):
        blk = S[32 * b:32 * b + 32]
        A = float(np.abs(blk).max())
        k = int(e[b]) - 127
        assert A <= 448.0 * 2.0 ** k and (e[b] == 0 or A > 448.0 * 2.0 ** (k - 1)), (b, A, k)
        assert np.array_equal(q[32 * b:32 * b + 32], F.narrow((blk.astype(np.float64) * 2.0 ** -k).astype(np.float32), kind))


def test_the_four_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "fmi_dev.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert lib.fmi_abi_version() == 1


def _tree_mx(op=0, dtype=12, alg=0, out_dtype=12, P=2, out_scales=True, n=64):
    """A call whose pointers are never read: it is refused by the host-side checks, or it is a call of n = 0 elements,
    which launches nothing whether or not a device is initialised."""
    lib = _lib.load()
    k = max(P, 1)
    bufs = [ctypes.create_string_buffer(64) for _ in range(2 * k)]
    ins = (ctypes.c_void_p * k)(*[ctypes.addressof(b) for b in bufs[:k]])
    scs = (ctypes.c_void_p * k)(*[ctypes.addressof(b) for b in bufs[k:]])
    out, osc = ctypes.create_string_buffer(256), ctypes.create_string_buffer(8)
    rc = lib.fmi_dev_reduce_tree_mx(op, dtype, alg, out_dtype, ctypes.addressof(out), ctypes.addressof(osc) if out_scales else None,
                                    ins, scs, P, 0, n, None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("kwargs,reason", [
    (dict(op=1), "op 1 is not valid here"),            # PROD
    (dict(op=2), "op 2 is not valid here"),            # MAX
    (dict(op=3), "op 3 is not valid here"),            # MIN
    (dict(alg=3), "alg 3 is a scan algorithm"),        # FMI_ALG_SCAN
    (dict(alg=4), "alg 4 is a scan algorithm"),        # FMI_ALG_SCAN_LTR
    (dict(dtype=2, out_dtype=2), "dtype 2 is not FMI_F8E4M3 or FMI_F8E5M2"),  # i32
    (dict(dtype=7, out_dtype=7), "dtype 7 is not FMI_F8E4M3 or FMI_F8E5M2"),  # u8
    (dict(dtype=0, out_dtype=0), "dtype 0 is not FMI_F8E4M3 or FMI_F8E5M2"),  # f32 elements
    (dict(dtype=12, out_dtype=13), "out_dtype 13"),    # the other 8-bit float
    (dict(dtype=13, out_dtype=12), "out_dtype 12"),
    (dict(out_dtype=11), "out_dtype 11"),              # bf16
    (dict(out_scales=False), "out_scales is NULL"),
    (dict(P=0), "P must be in"),
])
def test_reduce_tree_mx_validates_on_the_host(kwargs, reason):
    rc, msg = _tree_mx(**kwargs)
    assert rc == _lib.FMI_ERR_INVALID, (rc, msg)
    assert "fmi_dev_reduce_tree_mx" in msg or "P must be in" in msg, msg
    assert reason in msg, msg


def test_valid_arguments_pass_the_host_side_checks():
    """SUM and AVG, the flag (accepted and dropped), an f32 output without out_scales: none is refused by the host-side
    checks. The calls are of n = 0 elements, so that nothing is ever launched on these host pointers: past the checks
    the answer is FMI_ERR_NO_DEVICE where no device has been initialised (always, on a host without one) and FMI_OK
    where one has (this process ran GPU tests before)."""
    c = ctypes.c_int(-1)
    _lib.load().fmi_dev_count(ctypes.byref(c))
    for kwargs in (dict(), dict(op=5), dict(dtype=12 | 0x100), dict(dtype=13, out_dtype=13), dict(out_dtype=0, out_scales=False)):
        rc, msg = _tree_mx(n=0, **kwargs)
        assert rc in (_lib.FMI_ERR_NO_DEVICE, 0), (kwargs, rc, msg)
        if c.value <= 0:
            assert rc == _lib.FMI_ERR_NO_DEVICE, (kwargs, rc, msg)
    # the same arguments with PROD are refused at n = 0 too: the checks come first
    rc, msg = _tree_mx(n=0, op=1)
    assert rc == _lib.FMI_ERR_INVALID and "op 1 is not valid here" in msg, (rc, msg)


def test_quantize_and_dequantize_validate_on_the_host():
    lib = _lib.load()
    a, b, c = (ctypes.create_string_buffer(256) for _ in range(3))
    pa, pb, pc = (ctypes.addressof(x) for x in (a, b, c))
    for dtype, wide, reason in ((7, 0, "dtype 7 is not FMI_F8E4M3 or FMI_F8E5M2"), (2, 0, "dtype 2 is not"), (12, 1, "src_dtype 1 must be FMI_F32, FMI_F16 or FMI_BF16"),
                                (13, 13, "src_dtype 13 must be"), (12, 2, "src_dtype 2 must be")):
        assert lib.fmi_dev_mx_quantize(dtype, pa, pb, wide, pc, 32, None) == _lib.FMI_ERR_INVALID
        msg = _lib.last_error()
        assert "fmi_dev_mx_quantize" in msg and reason in msg, msg
    for dtype, wide, reason in ((6, 0, "dtype 6 is not FMI_F8E4M3 or FMI_F8E5M2"), (12, 1, "dst_dtype 1 must be FMI_F32, FMI_F16 or FMI_BF16"),
                                (13, 12, "dst_dtype 12 must be"), (12, 3, "dst_dtype 3 must be")):
        assert lib.fmi_dev_mx_dequantize(wide, pa, dtype, pb, pc, 32, None) == _lib.FMI_ERR_INVALID
        msg = _lib.last_error()
        assert "fmi_dev_mx_dequantize" in msg and reason in msg, msg
    # n = 0 succeeds, whatever the pointers, without a device
    assert lib.fmi_dev_mx_quantize(12, None, None, 0, None, 0, None) == 0
    assert lib.fmi_dev_mx_dequantize(11, None, 13, None, None, 0, None) == 0


def test_comm_call_validates_on_the_host():
    from fmi_amd.comm import Comm, Transport, unique_id

    lib = _lib.load()
    c0 = Comm(unique_id(Transport.LOCAL), 1, 0)
    h = ctypes.c_void_p(c0.handle)
    sc = ctypes.create_string_buffer(8)
    p = ctypes.addressof(sc)
    for args, reason in (((1, 12, 0, 12), "op 1 is not valid here"), ((2, 12, 0, 12), "op 2 is not valid here"), ((3, 13, 0, 13), "op 3 is not valid here"),
                         ((0, 12, 3, 12), "scan algorithm"), ((5, 12, 4, 12), "scan algorithm"), ((0, 12, 1, 12), "ALLREDUCE or REDUCE_LTR"),
                         ((0, 2, 0, 2), "dtype 2 is not"), ((0, 12, 0, 13), "out_dtype 13"), ((0, 13, 0, 10), "out_dtype 10")):
        assert lib.fmi_comm_allreduce_mx(h, *args, None, None, None, p, 8, None) == _lib.FMI_ERR_INVALID, args
        msg = _lib.last_error()
        assert "fmi_comm_allreduce_mx" in msg and reason in msg, (args, msg)
    assert lib.fmi_comm_allreduce_mx(h, 0, 12, 0, 12, None, None, None, None, 8, None) == _lib.FMI_ERR_INVALID
    assert "out_scales is NULL" in _lib.last_error()
    c0.destroy()


def test_python_refuses_wrong_buckets_before_the_library():
    """The Python checks need no device: buckets over raw pointers that are never dereferenced."""
    import fmi_amd
    from fmi_amd import Alg, Bucket, DType, Op

    def bk(n, dt):
        return Bucket(n, dt, ptr=4096)

    n = 70
    ins = [bk(n, DType.F8E4M3) for _ in range(2)]
    sc = [bk(3, DType.F8E8M0) for _ in range(2)]
    with pytest.raises(ValueError, match="needs F8E4M3 or F8E5M2 input buckets, got F32"):
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, bk(n, DType.F32), None, [bk(n, DType.F32)] * 2, sc)
    with pytest.raises(ValueError, match=r"ceil\(n / 32\) = 3 scale bytes for 70 elements, got 2"):
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, bk(n, DType.F8E4M3), bk(3, DType.F8E8M0), ins, [sc[0], bk(2, DType.F8E8M0)])
    with pytest.raises(ValueError, match="out_scales is missing"):
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, bk(n, DType.F8E4M3), None, ins, sc)
    with pytest.raises(ValueError, match="F8E8M0"):
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, bk(n, DType.F8E4M3), bk(3, DType.F32), ins, sc)
    with pytest.raises(ValueError, match="in their dtype or in F32"):
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, bk(n, DType.F8E5M2), bk(3, DType.F8E8M0), ins, sc)
    with pytest.raises(ValueError, match="F32, F16 or BF16"):
        fmi_amd.mx_quantize(bk(n, DType.F8E4M3), bk(3, DType.F8E8M0), bk(n, DType.F64))
    with pytest.raises(ValueError, match="scale bytes"):
        fmi_amd.mx_dequantize(bk(n, DType.BF16), bk(n, DType.F8E5M2), bk(4, DType.F8E8M0))
    assert fmi_amd.mx_blocks(0) == 0 and fmi_amd.mx_blocks(1) == 1 and fmi_amd.mx_blocks(32) == 1 and fmi_amd.mx_blocks(33) == 2
    assert int(DType.F8E8M0) == 14 and fmi_amd.device.itemsize_of(DType.F8E8M0) == 1
