"""Dev::reduce_tree_scaled of the C++ FMI surface on the GPU (fmi_amd/cpp/tests/test_fp8_scaled.cpp): inputs and scales
go in through files, the output and amax come back through files, compared bit for bit with tests/_fp8_scaled.py."""
import os
import subprocess

import numpy as np
import pytest

from tests import _fp8 as F
from tests import _fp8_scaled as FS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "cpp", "test_fp8_scaled")


def _exe():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fmi_amd", "cpp")], check=True)
    return EXE


@pytest.mark.parametrize("kind", F.KINDS)
def test_cpp_reduce_tree_scaled(tmp_path, kind):
    P, n = 5, 3 * 4096 + 7
    xs, s = [F.synthetic(kind, n, 7, p) for p in range(P)], FS.scales(P)
    np.concatenate(xs).tofile(tmp_path / "in.u8")
    s.tofile(tmp_path / "scales.f32")
    # the output scale travels as a decimal string: one that float parses to exactly the same value
    t_arg = repr(float(FS.T_OUT))
    assert np.float32(t_arg) == FS.T_OUT
    for alg, family, out, t in ((0, "allreduce", "f32", t_arg), (2, "reduce_ltr", "same", t_arg), (1, "reduce", "f32", "none")):
        res, am = tmp_path / f"res_{alg}", tmp_path / f"amax_{alg}"
        run = subprocess.run([_exe(), kind, str(alg), out, str(P), str(n), str(tmp_path / "in.u8"), str(tmp_path / "scales.f32"),
                              t, str(res), str(am)], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-2000:]
        want, want_amax, _ = FS.expected_scaled(family, kind, xs, s, None if t == "none" else FS.T_OUT, out)
        got = np.fromfile(res, np.uint8 if out == "same" else np.float32)
        FS.assert_out(got, want, kind, out, f"C++ {kind} {family} out={out}")
        FS.assert_amax(int(np.fromfile(am, np.uint32)[0]), want_amax, f"C++ {kind} {family}")
