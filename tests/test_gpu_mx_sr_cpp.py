"""Dev::reduce_tree_mx and Dev::mx_quantize with a trailing Dev::Sr (stochastic rounding) of the C++ FMI surface on the
GPU (fmi_amd/cpp/tests/test_mx_sr.cpp): inputs and scale bytes go in through files, the outputs come back through files,
compared bit for bit with tests/_mx_sr.py."""
import subprocess

import numpy as np
import pytest

from tests import _mx_sr as SR
from tests import _mxfp4 as M4
from tests.test_mx_sr_cpp import exe

pytestmark = pytest.mark.gpu

SEED, FIRST = 0xFEDCBA9876543210, 2 ** 35 - 64


@pytest.mark.parametrize("kind", SR.KINDS)
def test_cpp_reduce_tree_mx_sr(tmp_path, kind):
    P, n = 5, M4.N_TILE  # odd: an E2M1 bucket's last high nibble comes back 0
    xs, es = SR.visible_inputs(kind, n, P)
    np.concatenate([SR.element_bytes(x, kind) for x in xs]).tofile(tmp_path / "in.u8")
    np.concatenate(es).tofile(tmp_path / "scales.u8")
    for alg, family, op, opname in ((0, "allreduce", 0, "sum"), (2, "reduce_ltr", 5, "avg"), (1, "reduce", 0, "sum")):
        res, rsc = tmp_path / f"res_{alg}", tmp_path / f"rsc_{alg}"
        run = subprocess.run([exe(), "reduce", kind, str(op), str(alg), str(P), str(n), str(SEED), str(FIRST), str(tmp_path / "in.u8"),
                              str(tmp_path / "scales.u8"), str(res), str(rsc)], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-2000:]
        want, want_sc = SR.expected_sr(family, kind, xs, es, SEED, FIRST, opname)
        raw = np.fromfile(res, np.uint8)
        assert raw.size == SR.element_bytes(want, kind).size and (kind != "e2m1" or raw[-1] >> 4 == 0)
        assert np.array_equal(np.fromfile(rsc, np.uint8), want_sc), f"C++ {kind} {family} {opname}: scale bytes"
        assert np.array_equal(SR.codes_of(raw, kind, n), want), f"C++ {kind} {family} {opname}"


@pytest.mark.parametrize("kind", SR.KINDS)
def test_cpp_quantize_sr(tmp_path, kind):
    n = M4.N_TILE
    xs, es = SR.visible_inputs(kind, n, 8)
    S = SR.values("allreduce", kind, xs, es)
    S.tofile(tmp_path / "src.f32")
    q, sc = tmp_path / "q", tmp_path / "sc"
    run = subprocess.run([exe(), "quantize", kind, str(n), str(SEED), str(FIRST), str(tmp_path / "src.f32"), str(q), str(sc)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    want, want_sc = SR.quant_sr(S, kind, SEED, FIRST)
    assert np.array_equal(np.fromfile(sc, np.uint8), want_sc) and np.array_equal(SR.codes_of(np.fromfile(q, np.uint8), kind, n), want)
