"""FMI_OP_AVG without a device: the definition helper (tests/_avg.py) against torch CPU and against a division, the
C-ABI's validity checks (every one of them comes before a device is needed), the Python enums and the C++ surface."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import fmi_amd
from fmi_amd import _lib, fmi as ref_fmi
from tests import _avg as G
from tests import _half as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUM, AVG = 0, 5
F32, F64, I32, I16, F16, BF16, ACC = 0, 1, 2, 8, 10, 11, 0x100
ALLREDUCE, REDUCE, REDUCE_LTR, SCAN, SCAN_LTR = 0, 1, 2, 3, 4
ERR_INVALID = -1
N = 2061
TORCH = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16}


def last_error():
    return _lib.last_error()


def a_sum(kind, P, n=N, seed=7):
    """S of a P-peer allreduce in the value type (rank 0's)."""
    xs = [G.inputs(kind, n, seed, p) for p in range(P)]
    return G.sums("allreduce", kind, xs)[0], xs


def torch_bits(t, kind):
    if kind == "bf16":
        return t.view(torch.int16).numpy().view(np.uint16)
    if kind == "f16":
        return t.numpy().view(np.uint16)
    return t.numpy()


# ---- the definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 3, 8])
@pytest.mark.parametrize("kind", G.KINDS)
def test_helper_equals_torch_multiply(kind, P):
    """torch CPU's S * torch.tensor(1 / P, V) in the value type V (f32 for the 16-bit kinds, whose sum is widened:
    the reciprocal is rounded to V, never to the storage type), converted to the storage type once."""
    S, xs = a_sum(kind, P)
    V = torch.float64 if kind == "f64" else torch.float32
    want = (torch.from_numpy(np.array(S)) * torch.tensor(1 / P, dtype=V)).to(TORCH[kind])
    assert torch.from_numpy(np.array(S)).dtype == V
    G.assert_same(G.expected_avg("allreduce", kind, xs)[0], torch_bits(want, kind), kind, f"{kind} P={P}")


@pytest.mark.parametrize("P", [2, 4, 8, 16])
@pytest.mark.parametrize("kind", G.KINDS)
def test_helper_equals_division_at_powers_of_two(kind, P):
    S, xs = a_sum(kind, P)
    with np.errstate(all="ignore"):
        q = S / G.value_type(kind)(P)
    want = H.narrow(q, kind) if G.is_half(kind) else q
    G.assert_same(G.expected_avg("allreduce", kind, xs)[0], want, kind, f"{kind} P={P}")


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_helper_is_not_a_division_at_three(kind):
    """Multiplying by fl(1 / 3) differs from dividing by 3 in the last bit on some elements: nobody "fixes" the
    definition to a division without this failing."""
    S, xs = a_sum(kind, 3)
    fin = np.isfinite(S)
    with np.errstate(all="ignore"):
        q = S / G.value_type(kind)(3)
    got = G.expected_avg("allreduce", kind, xs)[0]
    assert (got[fin] != q[fin]).any()


def test_acc32_keeps_the_sum_in_f32():
    """f16, four peers holding 60000: the plain sum has overflowed to inf before anyone can scale it; the f32 sum
    240000 times 1/4 is exactly 60000."""
    xs = [H.from_float(np.full(9, 60000.0, np.float32), "f16") for _ in range(4)]
    plain = G.expected_avg("allreduce", "f16", xs)[0]
    acc = G.expected_avg("allreduce", "f16", xs, acc32=True)[0]
    assert (plain == 0x7C00).all() and np.array_equal(H.widen(acc, "f16"), np.full(9, 60000.0, np.float32))


def test_one_peer_is_the_copy():
    x = G.inputs("f32", 33, 3, 0)
    G.assert_same(G.expected_avg("allreduce", "f32", [x])[0], x, "f32")
    assert np.array_equal(G.expected_avg("reduce_ltr", "bf16", [H.inputs("bf16", 33, 3, 0)]), H.inputs("bf16", 33, 3, 0))


# ---- the C-ABI's validity checks, all before a device is needed -------------------------------------------------
def reduce_tree(op, dtype, alg, P=2):
    return _lib.load().fmi_dev_reduce_tree(op, dtype, alg, None, None, P, 0, ctypes.c_size_t(8), None)


def refused(rc, *words):
    msg = last_error()
    return rc == ERR_INVALID and "FMI_OP_AVG" in msg and all(w in msg for w in words)


def test_reduce_tree_takes_avg_on_float_dtypes_only():
    for dtype in (F32, F64, F16, BF16, F16 | ACC, BF16 | ACC):
        for alg in (ALLREDUCE, REDUCE, REDUCE_LTR):
            assert reduce_tree(AVG, dtype, alg) == ERR_INVALID
            assert "null buffer" in last_error(), last_error()  # past every check of op, dtype and alg
    for dtype in (I32, I16, 3, 7):
        assert refused(reduce_tree(AVG, dtype, ALLREDUCE), "integer", f"dtype {dtype}"), last_error()
    assert reduce_tree(AVG, F32 | ACC, ALLREDUCE) == ERR_INVALID and "FMI_ACC_F32" in last_error()


def test_reduce_tree_refuses_avg_at_scan_algorithms():
    for alg in (SCAN, SCAN_LTR):
        assert refused(reduce_tree(AVG, F32, alg), "op 5", "scan"), last_error()


def test_ids_four_and_nine_stay_unknown():
    for op in (4, 9):
        assert reduce_tree(op, F32, ALLREDUCE) == ERR_INVALID
        assert f"unknown op {op}" in last_error(), last_error()


def test_pairwise_and_scan_entry_points_refuse_avg():
    lib = _lib.load()
    n = ctypes.c_size_t(8)
    calls = {
        "fmi_dev_reduce_pair": lambda: lib.fmi_dev_reduce_pair(AVG, F32, None, None, n, None),
        "fmi_dev_reduce_pair_batch": lambda: lib.fmi_dev_reduce_pair_batch(AVG, F32, None, 0, None),
        "fmi_dev_combine": lambda: lib.fmi_dev_combine(AVG, F32, None, None, None, n, None),
        "fmi_host_reduce_pair": lambda: lib.fmi_host_reduce_pair(AVG, F32, None, None, n),
        "fmi_dev_scan_peers": lambda: lib.fmi_dev_scan_peers(AVG, F32, SCAN, None, None, 2, n, None),
    }
    for name, call in calls.items():
        assert refused(call(), name, "op 5"), (name, last_error())


def test_mean_scale_validates_without_a_device():
    lib = _lib.load()
    for dtype in (I32, I16, 4):
        assert lib.fmi_dev_mean_scale(dtype, None, ctypes.c_size_t(8), 2, None) == ERR_INVALID
        assert "integer" in last_error() and f"dtype {dtype}" in last_error(), last_error()
    assert lib.fmi_dev_mean_scale(BF16 | ACC, None, ctypes.c_size_t(8), 2, None) == ERR_INVALID
    assert lib.fmi_dev_mean_scale(F32, None, ctypes.c_size_t(8), 0, None) == ERR_INVALID and "P must be" in last_error()
    assert lib.fmi_dev_mean_scale(F32, None, ctypes.c_size_t(0), 3, None) == 0  # n = 0 succeeds
    assert lib.fmi_abi_version() == 1


# ---- Python ---------------------------------------------------------------------------------------------------
def test_python_enums():
    assert int(fmi_amd.Op.AVG) == AVG == int(ref_fmi.op.avg) and int(ref_fmi.op.custom) == 4
    assert 4 not in [int(o) for o in fmi_amd.Op]
    with open(os.path.join(ROOT, "include", "fmi_dev.h")) as f:
        assert "FMI_OP_AVG = 5" in f.read()
    assert callable(fmi_amd.device.mean_scale)


def test_reference_binding_takes_avg_on_doubles_only():
    check = ref_fmi.Communicator._check_avg
    f = ref_fmi.func(ref_fmi.op.avg)
    check(f, ref_fmi.types(ref_fmi.datatypes.double), "reduce")
    check(f, ref_fmi.types(ref_fmi.datatypes.double_list, 4), "allreduce")
    check(ref_fmi.func(ref_fmi.op.sum), ref_fmi.types(ref_fmi.datatypes.int), "scan")
    for t in (ref_fmi.types(ref_fmi.datatypes.int), ref_fmi.types(ref_fmi.datatypes.int_list, 4)):
        with pytest.raises(ValueError, match="double"):
            check(f, t, "allreduce")
    with pytest.raises(ValueError, match="scan"):
        check(f, ref_fmi.types(ref_fmi.datatypes.double), "scan")


# ---- C++ ------------------------------------------------------------------------------------------------------
def cpp_exe():
    exe = os.path.join(ROOT, "build", "cpp", "test_avg")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fmi_amd", "cpp")], check=True)
    return exe


def test_cpp_avg_cpu():
    """fmi_amd/cpp/tests/test_avg.cpp without arguments: Function<int>(Op::avg) throws, an avg Function's operator()
    and scan throw, reduce / allreduce over Loopback equal the sum finished by one multiply."""
    out = subprocess.run([cpp_exe()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    assert "0 failed checks" in out.stderr


def cpp_input_bits(p, n):
    """test_avg.cpp's input_bits, restated."""
    i = np.arange(n, dtype=np.uint64)
    M = np.uint64(0xFFFFFFFF)
    h = ((i * np.uint64(2654435761)) & M) ^ np.uint64(((p + 1) * 0x9E3779B9) & 0xFFFFFFFF)
    m = (h * np.uint64(2246822519)) & M
    bits = ((m >> np.uint64(31)) << np.uint64(31)) | ((np.uint64(107) + (h >> np.uint64(8)) % np.uint64(40)) << np.uint64(23)) \
        | (m & np.uint64(0x007FFFFF))
    return bits.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("P", [3, 4])
def test_cpp_loopback_allreduce_equals_the_helper(P):
    """Communicator::allreduce over Loopback with std::vector<float> and Op::avg: peer 0's bits equal the helper's."""
    n = 1031
    out = subprocess.run([cpp_exe(), "--dump", str(P), str(n)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    got = np.array([int(w, 16) for w in out.stdout.split()], np.uint32).view(np.float32)
    xs = [cpp_input_bits(p, n) for p in range(P)]
    G.assert_same(got, G.expected_avg("allreduce", "f32", xs)[0], "f32", f"C++ Loopback allreduce P={P}")
