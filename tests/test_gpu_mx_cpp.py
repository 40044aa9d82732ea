"""Dev::reduce_tree_mx, Dev::mx_quantize and Dev::mx_dequantize of the C++ FMI surface on the GPU
(fmi_amd/cpp/tests/test_mx.cpp): inputs and scale bytes go in through files, the outputs come back through files,
compared bit for bit with tests/_mx.py."""
import os
import subprocess

import numpy as np
import pytest

from tests import _fp8 as F
from tests import _mx as MX

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "cpp", "test_mx")


def _exe():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fmi_amd", "cpp")], check=True)
    return EXE


@pytest.mark.parametrize("kind", F.KINDS)
def test_cpp_reduce_tree_mx(tmp_path, kind):
    P, n = 5, 4096 + 96 + 17
    xs, es = MX.random_inputs(kind, n, P, seed=7, finite=True)
    np.concatenate(xs).tofile(tmp_path / "in.u8")
    np.concatenate(es).tofile(tmp_path / "scales.u8")
    for alg, family, op, opname, out in ((0, "allreduce", 0, "sum", "f32"), (2, "reduce_ltr", 5, "avg", "same"), (1, "reduce", 0, "sum", "same")):
        res, rsc = tmp_path / f"res_{alg}", tmp_path / f"rsc_{alg}"
        run = subprocess.run([_exe(), "reduce", kind, str(op), str(alg), out, str(P), str(n), str(tmp_path / "in.u8"),
                              str(tmp_path / "scales.u8"), str(res), str(rsc)], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-2000:]
        want, want_sc = MX.expected_mx(family, kind, xs, es, opname, out)
        got = np.fromfile(res, np.uint8 if out == "same" else np.float32)
        MX.assert_mx(got, np.fromfile(rsc, np.uint8) if out == "same" else None, want, want_sc, kind, out, f"C++ {kind} {family} {opname} out={out}")


@pytest.mark.parametrize("kind", F.KINDS)
def test_cpp_quantize_round_trip(tmp_path, kind):
    """float -> MX -> float through Dev::mx_quantize and Dev::mx_dequantize."""
    n = 4096 + 96 + 17
    S = MX.dequant(*[a[0] for a in MX.random_inputs(kind, n, 1, seed=9, finite=True)], kind) * np.float32(1.37)
    S.astype(np.float32).tofile(tmp_path / "src.f32")
    q, sc, back = tmp_path / "q", tmp_path / "sc", tmp_path / "back"
    run = subprocess.run([_exe(), "quantize", kind, str(n), str(tmp_path / "src.f32"), str(q), str(sc), str(back)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    want, want_sc = MX.quant(S, kind)
    MX.assert_mx(np.fromfile(q, np.uint8), np.fromfile(sc, np.uint8), want, want_sc, kind, "same", f"C++ {kind} quantize")
    MX.assert_f32_bits(np.fromfile(back, np.float32), MX.dequant(want, want_sc, kind), f"C++ {kind} dequantize")
