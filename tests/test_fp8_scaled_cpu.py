"""The scaled FP8 reduction without a GPU: the tests' own definition (tests/_fp8_scaled.py) against an f64 evaluation,
what its inputs can and cannot tell apart, the two symbols, and the host-side validation."""
import ctypes
import os
import re

import numpy as np
import pytest

from fmi_amd import _lib
from tests import _fp8 as F
from tests import _fp8_scaled as FS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fmi_dev_reduce_tree_scaled", "fmi_comm_allreduce_scaled")


def _inputs(kind, P, n=4096):
    return [F.synthetic(kind, n, 7, p) for p in range(P)]


@pytest.mark.parametrize("kind", F.KINDS)
def test_helper_equals_the_f64_definition(kind):
    """Small cases where every f32 operation can be redone in f64 and rounded once: a product of a 4-bit and a 24-bit
    significand and a sum of two f32 values of nearby exponents are exact in f64, so fl32(f64 result) is the IEEE f32
    result."""
    rng = np.random.default_rng(5)
    xs = [rng.integers(0, 256, 64).astype(np.uint8) for _ in range(3)]
    xs = [np.where(F.is_nan(x, kind) | np.isinf(F.widen(x, kind)), np.uint8(0x31), x) for x in xs]
    s = FS.scales(3)
    t = FS.T_OUT
    w = [F.widen(x, kind).astype(np.float64) for x in xs]
    v = [(w[p] * np.float64(s[p])).astype(np.float32) for p in range(3)]
    # reduce_ltr at P = 3: (v0 + v1) + v2
    S = ((v[0].astype(np.float64) + v[1].astype(np.float64)).astype(np.float32).astype(np.float64) + v[2].astype(np.float64)).astype(np.float32)
    y = (S.astype(np.float64) * np.float64(t)).astype(np.float32)
    out, amax, S_h = FS.expected_scaled("reduce_ltr", kind, xs, s, t, "f32")
    FS.assert_f32_bits(S_h, S, "S")
    FS.assert_f32_bits(out, y, "f32 out")
    assert amax == int(np.abs(S).view(np.uint32).max())
    out8, _, _ = FS.expected_scaled("reduce_ltr", kind, xs, s, t, "same")
    F.assert_bits(out8, F.narrow(y, kind), kind, "narrowed out")
    # P = 1 is not a copy
    o1, a1, _ = FS.expected_scaled("allreduce", kind, xs[:1], s[:1], t, "same")
    F.assert_bits(o1, F.narrow((v[0].astype(np.float64) * np.float64(t)).astype(np.float32), kind), kind, "P = 1")
    assert a1 == int(np.abs(v[0]).view(np.uint32).max())
    # t = None is 1.0
    o2, _, _ = FS.expected_scaled("reduce_ltr", kind, xs, s, None, "f32")
    FS.assert_f32_bits(o2, S, "t = None")


def test_amax_is_on_bits_and_nan_wins():
    S = np.array([1.0, -3.5, np.inf, 2.0], np.float32)
    assert FS.amax_bits(S) == 0x7F800000
    S[1] = np.nan
    assert (FS.amax_bits(S) & 0x7FFFFFFF) > 0x7F800000
    assert FS.fold_amax(0x40000000, FS.amax_bits(np.array([1.0], np.float32))) == 0x40000000


@pytest.mark.parametrize("kind", F.KINDS)
def test_fp8_output_cannot_pin_the_order_but_f32_output_can(kind):
    """Measured on these inputs (synthetic(kind, 4096, 7, p), FS.scales): the narrowed ALLREDUCE and REDUCE_LTR results
    agree in every element at P = 2..8 and in all but 0.1 % at P = 16; the f32 results differ in 20-67 % of elements
    at P = 3..16 (e4m3 25 / 34 / 48 / 67 % at P = 3 / 5 / 8 / 16). The floors are half the measured shares, so that
    nobody swaps in inputs on which a wrong order passes: the GPU order cases use the f32 output."""
    e4m3_floor = {3: 0.125, 5: 0.17, 8: 0.24, 16: 0.335}
    for P in (2, 3, 5, 8, 13, 16):
        xs, s = _inputs(kind, P), FS.scales(P)
        a8, _, Sa = FS.expected_scaled("allreduce", kind, xs, s, FS.T_OUT, "same")
        l8, _, Sl = FS.expected_scaled("reduce_ltr", kind, xs, s, FS.T_OUT, "same")
        same8 = float(np.mean(a8 == l8))
        diff32 = float(np.mean(Sa.view(np.uint32) != Sl.view(np.uint32)))
        print(f"{kind} P={P}: narrowed equal {same8:.4f}, f32 differ {diff32:.4f}")
        if P <= 8:
            assert same8 == 1.0, (kind, P, same8)
        else:
            assert same8 >= 0.99, (kind, P, same8)
        if P >= 3:
            floor = e4m3_floor.get(P, 0.10) if kind == "e4m3" else 0.10
            assert diff32 >= floor, (kind, P, diff32)


@pytest.mark.parametrize("kind,floor", [("e4m3", 0.08), ("e5m2", 0.025)])
def test_inputs_show_a_contracted_first_combine(kind, floor):
    """fma(widen(x0), s0, v1) against fl32(fl32(widen(x0) * s0) + v1): measured 16 % (e4m3) and 5 % (e5m2) of elements
    differ (11 % and 3 % as this test forms it, the first combine at P = 2); and 13-50 % of the products widen(x) * s are inexact
    (14 % of all e5m2 products, 34 % of e4m3's, up to 51 % for one peer). Floors at half the issue's figures."""
    xs, s = _inputs(kind, 2), FS.scales(2)
    v = FS.scaled_values(kind, xs, s)
    plain = (v[0] + v[1]).astype(np.float32)
    # both operands exact in f64 and their sum too (a 28-bit product and a 24-bit value within 2^6 of each other)
    fused = (F.widen(xs[0], kind).astype(np.float64) * np.float64(s[0]) + v[1].astype(np.float64)).astype(np.float32)
    share = float(np.mean(plain.view(np.uint32) != fused.view(np.uint32)))
    print(f"{kind}: contracted first combine differs in {share:.4f}")
    assert share >= floor, share
    # over the 16 peers together: a few of the scales end in zero bits and multiply exactly (peer 4: 0x3ffc9630)
    inexact = []
    for p in range(16):
        x = F.synthetic(kind, 4096, 7, p)
        exact = F.widen(x, kind).astype(np.float64) * np.float64(FS.scales(16)[p])
        inexact.append(exact.astype(np.float32).astype(np.float64) != exact)
    share = float(np.mean(inexact))
    print(f"{kind}: inexact products {share:.4f}, per peer at most {max(float(np.mean(i)) for i in inexact):.4f}")
    assert share >= 0.065, (kind, share)


def test_both_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "fmi_dev.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert lib.fmi_abi_version() == 1


def _tree_scaled(op=0, dtype=12, alg=0, out_dtype=12, P=2):
    """A call whose pointers are never read: every case here is refused by the host-side checks."""
    lib = _lib.load()
    k = max(P, 1)
    bufs = [ctypes.create_string_buffer(16) for _ in range(k)]
    ins = (ctypes.c_void_p * k)(*[ctypes.addressof(b) for b in bufs])
    out, sc = ctypes.create_string_buffer(64), ctypes.create_string_buffer(4 * k)
    rc = lib.fmi_dev_reduce_tree_scaled(op, dtype, alg, out_dtype, ctypes.addressof(out), ins, ctypes.addressof(sc), None, None,
                                        P, 0, 16, None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("kwargs,reason", [
    (dict(op=5), "fold 1 / P into out_scale"),         # FMI_OP_AVG
    (dict(op=1), "only FMI_OP_SUM"),                   # PROD
    (dict(alg=3), "scan algorithm"),                   # FMI_ALG_SCAN
    (dict(out_dtype=11), "out_dtype 11"),              # bf16
    (dict(dtype=0, out_dtype=0), "not FMI_F8E4M3 or FMI_F8E5M2"),  # f32 inputs
    (dict(P=0), "P must be in"),
])
def test_validation_is_host_side_and_names_the_reason(kwargs, reason):
    rc, msg = _tree_scaled(**kwargs)
    assert rc == _lib.FMI_ERR_INVALID, (rc, msg)
    assert reason in msg, msg


def test_acc_flag_is_accepted_and_dropped():
    """dtype | FMI_ACC_F32 passes the dtype check: with valid arguments the call gets as far as needing a device."""
    c = ctypes.c_int(-1)
    _lib.load().fmi_dev_count(ctypes.byref(c))
    if c.value > 0:
        pytest.skip("a device is visible; the refusal for lack of one is for GPU-less hosts")
    rc, msg = _tree_scaled(dtype=12 | 0x100)
    assert rc == _lib.FMI_ERR_NO_DEVICE, (rc, msg)


def test_comm_call_validates_on_the_host():
    from fmi_amd.comm import Comm, Transport, unique_id

    lib = _lib.load()
    c0 = Comm(unique_id(Transport.LOCAL), 1, 0)
    h = ctypes.c_void_p(c0.handle)
    assert lib.fmi_comm_allreduce_scaled(h, 5, 12, 0, 12, None, None, None, None, None, 8, None) == _lib.FMI_ERR_INVALID
    assert "fold 1 / P into out_scale" in _lib.last_error()
    assert lib.fmi_comm_allreduce_scaled(h, 0, 12, 1, 12, None, None, None, None, None, 8, None) == _lib.FMI_ERR_INVALID
    assert "ALLREDUCE or REDUCE_LTR" in _lib.last_error()
    assert lib.fmi_comm_allreduce_scaled(h, 0, 0, 0, 0, None, None, None, None, None, 8, None) == _lib.FMI_ERR_INVALID
    assert lib.fmi_comm_allreduce_scaled(h, 0, 13, 0, 10, None, None, None, None, None, 8, None) == _lib.FMI_ERR_INVALID
    c0.destroy()
