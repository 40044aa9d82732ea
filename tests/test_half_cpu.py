"""The 16-bit float element types (FMI_F16, FMI_BF16) without a GPU: the definition in tests/_half.py against
torch's CPU arithmetic on every bit pattern, the enumerators through the Python layers, and the C++ surface's
Dev::half / Dev::bfloat16 (fmi_amd/cpp/tests/test_half.cpp: conversions, dtypes, 3-peer host collectives)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _half as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "cpp", "test_half")


@pytest.fixture(scope="module")
def patterns():
    a, b = H.all_patterns(1 << 22)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@pytest.mark.parametrize("kind", H.KINDS)
def test_definition_matches_torch_cpu_on_all_patterns(patterns, kind):
    """widen / f32 op / narrow (and the selections for max / min) against torch CPU's own bfloat16 / float16
    arithmetic: all 65,536 patterns of a against 64 permutations of them as b, bit for bit, NaN <-> NaN."""
    import torch

    a, b = patterns
    tdt = torch.bfloat16 if kind == "bf16" else torch.float16
    ta = torch.from_numpy(a.view(np.int16).copy()).view(tdt)
    tb = torch.from_numpy(b.view(np.int16).copy()).view(tdt)
    want = {"sum": ta + tb, "prod": ta * tb, "max": torch.where(ta < tb, tb, ta), "min": torch.where(tb < ta, tb, ta)}
    for op in H.OPS:
        got = H.combine(op, a, b, kind)
        H.assert_bits(got, want[op].view(torch.int16).numpy().view(np.uint16), kind, op, f"{kind} {op}")
    # the NaN results the relaxation covers are a small minority: a NaN operand (2046 of the 65,536 f16 patterns,
    # 254 of the bf16 ones, on either side) or inf - inf
    nan = H.is_nan(H.combine("sum", a, b, kind), kind).mean()
    assert nan < 2 * (2046 if kind == "f16" else 254) / 65536 + 0.001, nan


def test_widen_narrow_round_trip_and_ties():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    for kind in H.KINDS:
        back = H.narrow(H.widen(bits, kind), kind)
        nan = H.is_nan(bits, kind)
        assert np.array_equal(back[~nan], bits[~nan])
        assert H.is_nan(back[nan], kind).all()
    f = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 2.0 ** -134, 3 * 2.0 ** -135, float.fromhex("0x1.FFp127")], np.float32)
    assert [int(v) for v in H.narrow(f, "bf16")] == [0x3F80, 0x3F82, 0x0000, 0x0001, 0x7F80]
    f = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -26, 65520.0], np.float32)
    assert [int(v) for v in H.narrow(f, "f16")] == [0x3C00, 0x3C02, 0x0000, 0x0001, 0x7C00]


def test_synthetic_fill_is_exact_and_in_range():
    for kind in H.KINDS:
        x = H.widen(H.synthetic(kind, 4099, seed=7, peer=3), kind)
        assert x.min() >= -1.0 and x.max() < 1.0 and len(np.unique(x)) > (100 if kind == "bf16" else 1000)


def test_python_layers_know_the_two_dtypes():
    import torch

    import fmi_amd
    from fmi_amd import DType, collectives
    from fmi_amd.device import dtype_of, itemsize_of

    assert int(DType.F16) == 10 and int(DType.BF16) == 11
    text = open(os.path.join(ROOT, "include", "fmi_dev.h")).read()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(FMI_[A-Z0-9_]+)\s*=\s*(\d+)", text)}
    assert consts["FMI_F16"] == 10 and consts["FMI_BF16"] == 11
    assert "#define FMI_DEV_ABI_VERSION 1" in text
    assert dtype_of(np.float16) is DType.F16
    assert dtype_of(np.uint16) is DType.U16 and dtype_of(np.zeros(3, np.uint16)) is DType.U16
    assert itemsize_of(DType.BF16) == 2 and itemsize_of(np.float16) == 2
    assert collectives._dtype(torch.empty(1, dtype=torch.float16)) is DType.F16
    assert collectives._dtype(torch.empty(1, dtype=torch.bfloat16)) is DType.BF16
    with pytest.raises(TypeError, match="f16"):
        dtype_of(np.complex64)
    assert fmi_amd.DType is DType


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fmi_amd", "cpp")], check=True)
    return EXE


def test_cpp_half_types_host(exe):
    """Dev::dtype_of, float round trips of Dev::half / Dev::bfloat16 (ties, overflow, NaN, subnormals) and 3-peer
    Loopback allreduce / scan of Data<std::vector<Dev::bfloat16>> (sum, max) on the host combine path against
    values written out from the definition."""
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    assert "0 failed checks" in out.stderr


def test_cpp_known_answers_are_the_definitions():
    """The values written out in test_half.cpp are the oracle simulation's, with f = this helper's combine."""
    from oracle import fmi_oracle as orc

    src = open(os.path.join(ROOT, "fmi_amd", "cpp", "tests", "test_half.cpp")).read()

    def table(name):
        body = re.search(name + r" = \{(.*?)\};", src, re.S).group(1)
        return [np.array([int(v, 16) for v in re.findall(r"0x[0-9A-Fa-f]+", row)], np.uint16)
                for row in re.findall(r"\{([^{}]*)\}", body)]

    xs = table("kIn")
    assert len(xs) == 3
    for op, ar_name, sc_name in (("sum", "kSumAllreduce", "kSumScan"), ("max", "kMaxAllreduce", "kMaxScan")):
        ar, _ = orc.allreduce(xs, H.combiner(op, "bf16"))
        sc, _ = orc.scan(xs, H.combiner(op, "bf16"))
        for p in range(3):
            assert np.array_equal(table(ar_name)[p], ar[p]), (op, "allreduce", p)
            assert np.array_equal(table(sc_name)[p], sc[p]), (op, "scan", p)
