"""The C++ 8-bit float element types (FMI::Dev::float8_e4m3 / float8_e5m2, fmi_amd/cpp/tests/test_fp8.cpp) without a
device: their own checks, and their software narrowing / widening against tests/_fp8.py on the boundary set and on all
256 patterns."""
import os
import subprocess

import numpy as np

from tests import _fp8 as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "cpp", "test_fp8")


def _exe():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fmi_amd", "cpp")], check=True)
    return EXE


def test_cpp_fp8_cpu():
    out = subprocess.run([_exe()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    assert "0 failed checks" in out.stderr


def test_cpp_narrowing_equals_the_definition(tmp_path):
    x = F.boundary_f32()
    src, dst = tmp_path / "in.f32", tmp_path / "out.u8"
    x.tofile(src)
    subprocess.run([_exe(), "--narrow", str(src), str(dst)], check=True, timeout=300)
    got = np.fromfile(dst, np.uint8)
    assert got.size == 2 * x.size
    for k, kind in enumerate(F.KINDS):
        F.assert_bits(got[k * x.size:(k + 1) * x.size], F.narrow(x, kind), kind, f"C++ narrowing to {kind}")


def test_cpp_widening_equals_the_definition(tmp_path):
    dst = tmp_path / "out.f32"
    subprocess.run([_exe(), "--widen", str(dst)], check=True, timeout=300)
    got = np.fromfile(dst, np.float32)
    bits = np.arange(256, dtype=np.uint8)
    for k, kind in enumerate(F.KINDS):
        g, w = got[256 * k:256 * (k + 1)], F.widen(bits, kind)
        assert np.all((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))), kind
