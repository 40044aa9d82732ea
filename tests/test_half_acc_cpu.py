"""FMI_ACC_F32 without a device: the C-ABI's validation of the flag, the Python keyword, the C++ layer's CPU side,
and that the inputs of tests/test_gpu_half_acc.py tell a wrong order or a per-combine rounding from the right
result (measured on the oracle alone; each bound is well below the measured fraction quoted beside it)."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import fmi_amd
from fmi_amd import _lib, device as fdev
from fmi_amd.comm import Comm
from oracle import fmi_oracle as orc
from tests import _half as H
from tests import _half_acc as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, I16, BF16, F16, ACC = 0, 8, 11, 10, 0x100
ERR_INVALID = -1
N = 2061


def last_error():
    return _lib.last_error()


def test_constant_matches_header():
    assert fdev.ACC_F32 == ACC == fmi_amd.ACC_F32
    with open(os.path.join(ROOT, "include", "fmi_dev.h")) as f:
        assert "#define FMI_ACC_F32 0x100" in f.read()


@pytest.mark.parametrize("entry", ["fmi_dev_reduce_tree", "fmi_dev_scan_peers"])
def test_abi_validates_the_flag_without_a_device(entry):
    """The flag is accepted on the two 16-bit float dtypes (the call then fails on its null buffers, not on the
    dtype) and refused, naming the dtype, on every other one."""
    lib = _lib.load()
    fn = getattr(lib, entry)
    alg = 0 if entry == "fmi_dev_reduce_tree" else 3

    def call(dtype):
        if entry == "fmi_dev_reduce_tree":
            return fn(0, dtype, alg, None, None, 2, 0, ctypes.c_size_t(8), None)
        return fn(0, dtype, alg, None, None, 2, ctypes.c_size_t(8), None)

    for dtype in (BF16 | ACC, F16 | ACC):
        assert call(dtype) == ERR_INVALID
        assert "null buffer" in last_error() and "dtype" not in last_error(), last_error()
    for dtype in (F32 | ACC, I16 | ACC):
        assert call(dtype) == ERR_INVALID
        assert "dtype" in last_error() and str(dtype) in last_error() and "FMI_ACC_F32" in last_error(), last_error()
    assert call(BF16 | 0x200) == ERR_INVALID and "dtype" in last_error()


def test_python_keyword():
    for fn in (fmi_amd.reduce_tree, fmi_amd.scan_peers, Comm.allreduce, Comm.allreduce_host, Comm.reduce, Comm.scan):
        p = inspect.signature(fn).parameters["accumulate_f32"]
        assert p.default is False
    assert fdev.acc_dtype(fdev.DType.BF16, True) == BF16 | ACC and fdev.acc_dtype(fdev.DType.F16, True) == F16 | ACC
    assert fdev.acc_dtype(fdev.DType.BF16, False) == BF16

    class Fake:  # stands in for a Bucket: the keyword is checked before anything touches the library or a pointer
        dtype, n, ptr = fdev.DType.F32, 8, 0

    with pytest.raises(ValueError, match="F16 or BF16"):
        fmi_amd.reduce_tree(fmi_amd.Op.SUM, fmi_amd.Alg.ALLREDUCE, Fake(), [Fake(), Fake()], accumulate_f32=True)
    with pytest.raises(ValueError, match="F16 or BF16"):
        fmi_amd.scan_peers(fmi_amd.Op.SUM, fmi_amd.Alg.SCAN, [Fake(), Fake()], [Fake(), Fake()], accumulate_f32=True)
    with pytest.raises(ValueError, match="F16 or BF16"):
        Comm.allreduce(None, fmi_amd.Op.SUM, Fake(), Fake(), accumulate_f32=True)
    with pytest.raises(ValueError, match="F16 or BF16"):
        Comm.allreduce_host(None, fmi_amd.Op.SUM, np.zeros(8, np.float32), np.zeros(8, np.float32), accumulate_f32=True)


@pytest.mark.parametrize("kind", H.KINDS)
def test_cancel_inputs_tell_the_orders_apart(kind):
    for P in (5, 17):
        xs = A.cancel_inputs(kind, N, P, 41)
        ar = A.expected_acc("allreduce", kind, "sum", xs)[0]
        ltr = A.expected_acc("reduce_ltr", kind, "sum", xs)
        assert A.differing(ar, ltr, kind) >= 0.5  # measured 0.94 - 1.00
        r0 = A.expected_acc("reduce", kind, "sum", xs, root=0)[0]
        r5 = A.expected_acc("reduce", kind, "sum", xs, root=5 if P > 5 else 3)[0]
        assert A.differing(r0, r5, kind) >= 0.5  # measured 0.75 (P = 5, root 3), 0.95 (P = 17, root 5)
    xs = A.cancel_inputs(kind, N, 17, 41)
    sc, sl = A.expected_acc("scan", kind, "sum", xs), A.expected_acc("scan_ltr", kind, "sum", xs)
    assert np.mean([A.differing(sc[r], sl[r], kind) for r in range(17)]) >= 0.10  # measured 0.24


@pytest.mark.parametrize("kind", H.KINDS)
def test_inputs_tell_f32_accumulation_from_per_combine_rounding(kind):
    xs = [H.inputs(kind, N, 31, p) for p in range(8)]
    for op, bound in (("sum", 0.02), ("prod", 0.20)):  # measured f16 0.057 / 0.42, bf16 0.049 / 0.49
        acc = A.expected_acc("allreduce", kind, op, xs)[0]
        plain = orc.allreduce(xs, H.combiner(op, kind))[0][0]
        assert A.differing(acc, plain, kind) >= bound


def test_two_peers_are_one_combine():
    """P = 2 is a single combine, already "widen, op, round once": acc32 and the plain definition agree on every pair
    of edge values, which is what pins the kernels' widen / narrow code on all 65,536 patterns on the GPU."""
    for kind in H.KINDS:
        a, b = H.edge_values(kind)
        for op in ("sum", "prod"):
            H.assert_bits(A.expected_acc("allreduce", kind, op, [a, b])[0], H.combine(op, a, b, kind), kind, op)


def test_cpp_half_acc_cpu():
    """fmi_amd/cpp/tests/test_half_acc.cpp without arguments: Function carries Accumulate::f32 into device_op for
    Dev::half / Dev::bfloat16, a wrong element type throws, and a Loopback allreduce is unchanged by it."""
    exe = os.path.join(ROOT, "build", "cpp", "test_half_acc")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fmi_amd", "cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    assert "0 failed checks" in out.stderr
