"""Dev::mx_quantize_sr_host and the argument checks of the Dev::Sr overloads of the C++ FMI surface
(fmi_amd/cpp/tests/test_mx_sr.cpp), without a GPU: the host quantization through files against tests/_mx_sr.py, and
every refusal the header or the library makes before a device is needed."""
import os
import subprocess

import numpy as np
import pytest

from tests import _mx_sr as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "cpp", "test_mx_sr")


def exe():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fmi_amd", "cpp")], check=True)
    return EXE


@pytest.mark.parametrize("kind", SR.KINDS)
def test_cpp_host_quantize_equals_the_definition(tmp_path, kind):
    n = 1001  # a ragged last block; odd for E2M1
    xs, es = SR.visible_inputs(kind, n, 8)
    S = SR.values("allreduce", kind, xs, es)
    S[64:96] = 0
    S[100] = np.nan
    S.tofile(tmp_path / "src.f32")
    for seed, first in ((0x0123456789ABCDEF, 0), (2 ** 64 - 1, 2 ** 35 - 64)):
        run = subprocess.run([exe(), "host", kind, str(n), str(seed), str(first), str(tmp_path / "src.f32"), str(tmp_path / "out"),
                              str(tmp_path / "sc")], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-2000:]
        want, want_sc = SR.quant_sr(S, kind, seed, first)
        raw = np.fromfile(tmp_path / "out", np.uint8)
        assert raw.size == SR.element_bytes(want, kind).size
        assert np.array_equal(np.fromfile(tmp_path / "sc", np.uint8), want_sc), (kind, seed)
        assert np.array_equal(SR.codes_of(raw, kind, n), want), (kind, seed)
        assert want_sc[3] == 255 and (want != SR.quant_rne(S, kind)[0]).mean() > 0.05


def test_cpp_argument_checks():
    run = subprocess.run([exe(), "checks"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "checks ok" in run.stdout and "ACCEPTED" not in run.stdout, (run.stdout[-3000:], run.stderr[-2000:])
    said = {line.split(":", 1)[0][len("refused "):]: line for line in run.stdout.splitlines() if line.startswith("refused ")}
    for what, text in (("a seed bucket of two words", "one std::uint64_t"), ("a null seed", "seed is NULL"), ("a misaligned seed", "8-byte aligned"),
                       ("first = 16", "multiple of 32"),
                       ("first + n wraps", "wraps"), ("op MAX", "FMI_OP_SUM"), ("short out_scales", "(n + 31) / 32"),
                       ("quantize, first = 48", "multiple of 32"), ("quantize, a seed bucket of two words", "one std::uint64_t"),
                       ("quantize, size mismatch", "size mismatch"), ("host, first = 8", "multiple of 32")):
        assert text in said[what], said[what]
