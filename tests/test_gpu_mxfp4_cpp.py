"""Dev::reduce_tree_mx, Dev::mx_quantize and Dev::mx_dequantize on MXFP4 buckets (Dev::float4_e2m1x2) of the C++ FMI
surface on the GPU (fmi_amd/cpp/tests/test_mxfp4.cpp): packed inputs and scale bytes go in through files, the outputs
come back through files, compared bit for bit with tests/_mxfp4.py. And the header's host widen / narrow of a nibble."""
import os
import subprocess

import numpy as np
import pytest

from tests import _fp8 as F
from tests import _mxfp4 as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "cpp", "test_mxfp4")


def _exe():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fmi_amd", "cpp")], check=True)
    return EXE


def test_cpp_reduce_tree_mxfp4(tmp_path):
    P, n = 5, M.N_TILE  # odd: the last byte's high nibble comes back 0
    xs, es = M.random_inputs(n, P, 7, 112, 142)
    np.concatenate([M.pack(x) for x in xs]).tofile(tmp_path / "in.u8")
    np.concatenate(es).tofile(tmp_path / "scales.u8")
    for alg, family, op, opname, out in ((0, "allreduce", 0, "sum", "f32"), (2, "reduce_ltr", 5, "avg", "same"), (1, "reduce", 0, "sum", "same")):
        res, rsc = tmp_path / f"res_{alg}", tmp_path / f"rsc_{alg}"
        run = subprocess.run([_exe(), "reduce", str(op), str(alg), out, str(P), str(n), str(tmp_path / "in.u8"),
                              str(tmp_path / "scales.u8"), str(res), str(rsc)], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-2000:]
        want, want_sc = M.expected(family, xs, es, opname, out)
        if out == "f32":
            M.assert_mx(np.fromfile(res, np.float32), None, want, None, out, f"C++ {family} {opname}")
        else:
            raw = np.fromfile(res, np.uint8)
            assert raw.size == (n + 1) // 2 and raw[-1] >> 4 == 0
            M.assert_mx(M.unpack(raw, n), np.fromfile(rsc, np.uint8), want, want_sc, out, f"C++ {family} {opname}")


def test_cpp_quantize_round_trip(tmp_path):
    """float -> MXFP4 -> float through Dev::mx_quantize and Dev::mx_dequantize."""
    n = M.N_TILE
    xs, es = M.random_inputs(n, 1, 9)
    S = (M.dequant(xs[0], es[0]) * np.float32(1.37)).astype(np.float32)
    S.tofile(tmp_path / "src.f32")
    q, sc, back = tmp_path / "q", tmp_path / "sc", tmp_path / "back"
    run = subprocess.run([_exe(), "quantize", str(n), str(tmp_path / "src.f32"), str(q), str(sc), str(back)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    want, want_sc = M.quant(S)
    M.assert_mx(M.unpack(np.fromfile(q, np.uint8), n), np.fromfile(sc, np.uint8), want, want_sc, "same", "C++ quantize")
    M.assert_mx(np.fromfile(back, np.float32), None, M.dequant(want, want_sc), None, "f32", "C++ dequantize")


def test_cpp_host_widen_and_narrow(tmp_path):
    """Dev::float4_e2m1x2::narrow on the f32 boundary set within |y| <= 6, and widen of the 16 codes (no device)."""
    b = F.boundary_f32()
    b = b[np.isfinite(b) & (np.abs(b) <= 6)]
    b.tofile(tmp_path / "src.f32")
    run = subprocess.run([_exe(), "host", str(b.size), str(tmp_path / "src.f32"), str(tmp_path / "codes"), str(tmp_path / "table")],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    assert np.array_equal(np.fromfile(tmp_path / "codes", np.uint8), M.narrow(b))
    assert np.array_equal(np.fromfile(tmp_path / "table", np.float32).view(np.uint32), M.TABLE.view(np.uint32))
