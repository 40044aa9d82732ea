"""The 8-bit float dtypes without a device: tests/_fp8.py (the definition every FP8 GPU test compares against) pinned
to torch CPU's float8 tensors, the Python enum against the header, and the C-ABI's host-side argument validation
(fmi_dev_convert, FMI_ACC_F32 on the two new dtypes)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fmi_amd
from fmi_amd import _lib, device as fdev
from tests import _fp8 as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
F32, F64, I32, U8, F16, BF16, E4M3, E5M2, ACC = 0, 1, 2, 7, 10, 11, 12, 13, 0x100
ERR_INVALID = -1


def t_widen(bits: np.ndarray, kind: str) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint8)).view(TORCH[kind]).to(torch.float32).numpy()


def t_narrow(x: np.ndarray, kind: str) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(TORCH[kind]).view(torch.uint8).numpy()


def same(a, b, kind):
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    return bool(np.all((a == b) | (F.is_nan(a, kind) & F.is_nan(b, kind))))


@pytest.mark.parametrize("kind", F.KINDS)
def test_widen_all_patterns_equals_torch(kind):
    bits = np.arange(256, dtype=np.uint8)
    got, want = F.widen(bits, kind), t_widen(bits, kind)
    assert np.all((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    assert int(np.isnan(got).sum()) == (2 if kind == "e4m3" else 6)
    assert np.nanmax(np.where(np.isinf(got), np.nan, got)) == F.MAX_FINITE[kind]


@pytest.mark.parametrize("kind", F.KINDS)
def test_narrow_boundary_set_equals_torch(kind):
    x = F.boundary_f32()
    assert x.size == 393216
    got, want = F.narrow(x, kind), t_narrow(x, kind)
    assert same(got, want, kind)
    assert len(np.unique(want)) == (256 if kind == "e4m3" else 252)  # the set reaches every byte a narrowing can give
    # widening is exact, so narrowing a widened pattern is the identity (NaN as a class)
    bits = np.arange(256, dtype=np.uint8)
    assert same(F.narrow(F.widen(bits, kind), kind), bits, kind)


def test_the_values_the_header_names():
    e4 = lambda v: int(F.narrow(np.array([v], np.float32), "e4m3")[0])  # noqa: E731
    e5 = lambda v: int(F.narrow(np.array([v], np.float32), "e5m2")[0])  # noqa: E731
    assert e4(464.0) == 0x7E and e4(465.0) == 0x7F and e4(np.inf) == 0x7F and e4(-np.inf) == 0xFF
    assert e5(61440.0) == 0x7C and e5(61439.9) == 0x7B and e5(-np.inf) == 0xFC and e5(1e9) == 0x7C
    assert e4(-0.0) == 0x80 and e5(-0.0) == 0x80


@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("op", F.OPS)
def test_combine_table_equals_torch(kind, op):
    """Every (a, b) of the 256 x 256 table: widen, op in f32, narrow, all by torch; max / min select bytes."""
    a, b = F.table_pairs()
    ta, tb = torch.from_numpy(t_widen(a, kind)), torch.from_numpy(t_widen(b, kind))
    if op == "sum":
        want = (ta + tb).to(TORCH[kind]).view(torch.uint8).numpy()
    elif op == "prod":
        want = (ta * tb).to(TORCH[kind]).view(torch.uint8).numpy()
    elif op == "max":
        want = np.where((ta < tb).numpy(), b, a)
    else:
        want = np.where((tb < ta).numpy(), b, a)
    got = F.combine(op, a, b, kind)
    if op in ("max", "min"):
        assert np.array_equal(got, want)  # selections: the operand's own byte, NaN payloads and +-0 included
    else:
        assert same(got, want, kind)


def test_e5m2_sum_is_not_always_exact_in_f32_and_e4m3_is():
    """The f32 intermediate is part of the definition (include/fmi_dev.h)."""
    for kind, exact in (("e4m3", True), ("e5m2", False)):
        a, b = F.table_pairs()
        wa, wb = F.widen(a, kind).astype(np.float64), F.widen(b, kind).astype(np.float64)
        ok = np.isfinite(wa) & np.isfinite(wb)
        with np.errstate(invalid="ignore"):  # inf - inf among the non-finite patterns, masked out below
            s32, s64 = (wa.astype(np.float32) + wb.astype(np.float32)).astype(np.float64), wa + wb
        assert bool(np.all(s32[ok] == s64[ok])) is exact


@pytest.mark.parametrize("kind", F.KINDS)
def test_synthetic_is_exact_and_in_range(kind):
    x = F.synthetic(kind, 4096, seed=5, peer=3)
    v = F.widen(x, kind)
    step = 0.125 if kind == "e4m3" else 0.25
    assert v.min() >= -1.0 and v.max() < 1.0 and np.all(v / step == np.round(v / step))
    assert len(np.unique(x)) == (16 if kind == "e4m3" else 8)
    assert np.array_equal(F.synthetic(kind, 100, 5, 3, start=50), x[50:150])


def test_cancel_inputs_tell_the_orders_apart():
    """The inputs of the GPU test's cancelling case. e5m2: the ALLREDUCE and REDUCE_LTR expectations differ on the SUM
    inputs, so a wrong bracketing cannot hide behind the final rounding. e4m3: an f32 SUM of e4m3 values is exact in
    every order (_fp8.cancel_inputs), so there the SUM inputs tell f32 accumulation from per-combine rounding and the
    PROD inputs of _fp8.order_inputs tell the orders apart, for both formats, through the f32 range."""
    for kind in F.KINDS:
        xs = F.cancel_inputs(kind, 2061, 8, seed=11)
        a = F.expected_acc("allreduce", kind, "sum", xs)[0]
        b = F.expected_acc("reduce_ltr", kind, "sum", xs)
        assert not F.is_nan(a, kind).any() and not F.is_nan(b, kind).any()
        if kind == "e5m2":
            assert (a != b).mean() > 0.3, (kind, (a != b).mean())  # measured 0.67
        else:
            assert np.array_equal(a, b)
            plain = F.expected_plain("allreduce", kind, "sum", xs)[0]
            assert (a != plain).mean() > 0.5, (kind, (a != plain).mean())  # measured 0.83
        xs = F.order_inputs(kind, 2061, 16, seed=12)
        a = F.expected_acc("allreduce", kind, "prod", xs)[0]
        b = F.expected_acc("reduce_ltr", kind, "prod", xs)
        differ = ~((a == b) | (F.is_nan(a, kind) & F.is_nan(b, kind)))
        assert not F.is_nan(a, kind).any() and differ.mean() > 0.7  # three elements in four, by construction


def test_overflow_inputs_show_saturation_and_per_combine_rounding():
    for kind in F.KINDS:
        for P in (5, 8):
            xs = F.overflow_inputs(kind, 515, P, seed=4)
            ws = [F.widen(x, kind).astype(np.float64) for x in xs]
            assert max(np.abs(w).max() for w in np.cumsum(ws, axis=0)) > F.MAX_FINITE[kind]  # a partial is out of range
            acc = F.expected_acc("reduce_ltr", kind, "sum", xs)
            assert not F.is_nan(acc, kind).any() and np.abs(F.widen(acc, kind)).max() < 8
            plain = F.expected_plain("reduce_ltr", kind, "sum", xs)
            bad = F.is_nan(plain, kind) | np.isinf(F.widen(plain, kind))
            assert bad.all()  # per-combine narrowing: the overflow shows (NaN for e4m3, inf - inf = NaN for e5m2)


def test_python_enum_and_header_agree():
    text = open(os.path.join(ROOT, "include", "fmi_dev.h")).read()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(FMI_[A-Z0-9_]+)\s*=\s*(\d+)", text)}
    assert consts["FMI_F8E4M3"] == 12 == int(fmi_amd.DType.F8E4M3) == E4M3
    assert consts["FMI_F8E5M2"] == 13 == int(fmi_amd.DType.F8E5M2) == E5M2
    assert fdev.itemsize_of(fmi_amd.DType.F8E4M3) == 1 == fdev.itemsize_of(fmi_amd.DType.F8E5M2)
    assert fdev.dtype_of(np.uint8) == fmi_amd.DType.U8  # np.uint8 alone keeps meaning U8
    assert fdev.acc_dtype(fmi_amd.DType.F8E4M3, True) == E4M3 | ACC and fdev.acc_dtype(fmi_amd.DType.F8E5M2, True) == E5M2 | ACC
    assert "fmi_dev_convert" in _lib.SIGNATURES and callable(fmi_amd.convert)
    assert _lib.load().fmi_abi_version() == 1


def test_convert_validates_its_dtypes_without_a_device():
    lib = _lib.load()
    n0, n8 = ctypes.c_size_t(0), ctypes.c_size_t(8)
    for d in (F32, F16, BF16, E4M3, E5M2):
        for s in (F32, F16, BF16, E4M3, E5M2):
            assert lib.fmi_dev_convert(d, None, s, None, n0, None) == 0  # n = 0 succeeds, before any device is needed
            assert lib.fmi_dev_convert(d, None, s, None, n8, None) == ERR_INVALID and "null buffer" in _lib.last_error()
    for bad in (F64, I32, U8, E4M3 | ACC, BF16 | ACC, 14, -1):
        for args in ((bad, None, F32, None), (E4M3, None, bad, None)):
            assert lib.fmi_dev_convert(*args, n0, None) == ERR_INVALID
            assert "fmi_dev_convert" in _lib.last_error() and str(bad) in _lib.last_error(), _lib.last_error()


@pytest.mark.parametrize("entry", ["fmi_dev_reduce_tree", "fmi_dev_scan_peers"])
def test_abi_accepts_the_flag_on_the_8bit_floats_without_a_device(entry):
    """As for f16 / bf16: with the flag the call fails on its null buffers, not on the dtype; dtype 14 stays unknown."""
    fn = getattr(_lib.load(), entry)

    def call(dtype):
        if entry == "fmi_dev_reduce_tree":
            return fn(0, dtype, 0, None, None, 2, 0, ctypes.c_size_t(8), None)
        return fn(0, dtype, 3, None, None, 2, ctypes.c_size_t(8), None)

    for dtype in (E4M3, E5M2, E4M3 | ACC, E5M2 | ACC):
        assert call(dtype) == ERR_INVALID
        assert "null buffer" in _lib.last_error() and "dtype" not in _lib.last_error(), _lib.last_error()
    for dtype in (14, 14 | ACC, U8 | ACC):
        assert call(dtype) == ERR_INVALID and "dtype" in _lib.last_error()


def test_pairwise_calls_accept_and_drop_the_flag():
    """n = 0 succeeds whatever else: only the dtype argument is looked at before that."""
    lib = _lib.load()
    for dtype in (E4M3, E5M2, E4M3 | ACC, E5M2 | ACC):
        assert lib.fmi_host_reduce_pair(0, dtype, None, None, ctypes.c_size_t(0)) == 0
    assert lib.fmi_host_reduce_pair(0, U8 | ACC, None, None, ctypes.c_size_t(0)) == ERR_INVALID
    assert lib.fmi_host_reduce_pair(5, E4M3, None, None, ctypes.c_size_t(0)) == ERR_INVALID  # no pairwise mean
    # fmi_dev_mean_scale: the plain dtypes alone
    assert lib.fmi_dev_mean_scale(E4M3, None, ctypes.c_size_t(0), 3, None) == 0
    assert lib.fmi_dev_mean_scale(E4M3 | ACC, None, ctypes.c_size_t(0), 3, None) == ERR_INVALID


def test_python_keyword_accepts_the_8bit_floats():
    class Fake:
        dtype, n, ptr = fdev.DType.U8, 8, 0

    with pytest.raises(ValueError, match="accumulate_f32 needs.*got U8"):  # np.uint8 alone is U8: refused
        fmi_amd.reduce_tree(fmi_amd.Op.SUM, fmi_amd.Alg.ALLREDUCE, Fake(), [Fake(), Fake()], accumulate_f32=True)
    # accepted on the two 8-bit floats: the keyword passes the check and the call reaches the library, which answers
    # the null pointers (FmiError), not the dtype
    for dt in (fdev.DType.F8E4M3, fdev.DType.F8E5M2):
        Fake.dtype = dt
        with pytest.raises(fmi_amd.FmiError, match="null"):
            fmi_amd.reduce_tree(fmi_amd.Op.SUM, fmi_amd.Alg.ALLREDUCE, Fake(), [Fake(), Fake()], accumulate_f32=True)


def test_torch_glue_maps_the_8bit_floats():
    from fmi_amd import collectives
    assert collectives._TORCH_DTYPE[torch.float8_e4m3fn] == fmi_amd.DType.F8E4M3
    assert collectives._TORCH_DTYPE[torch.float8_e5m2] == fmi_amd.DType.F8E5M2
    assert collectives._TORCH_DTYPE[torch.uint8] == fmi_amd.DType.U8
