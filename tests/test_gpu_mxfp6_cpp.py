"""Dev::reduce_tree_mx, Dev::mx_quantize and Dev::mx_dequantize on MXFP6 buckets (Dev::float6_e2m3_packed /
Dev::float6_e3m2_packed) of the C++ FMI surface (fmi_amd/cpp/tests/test_mxfp6.cpp): packed inputs and scale bytes go in
through files, the outputs come back through files, compared bit for bit with tests/_mxfp6.py. The header's host pack /
widen / narrow and Dev::mx_quantize_sr_host need no device."""
import os
import subprocess

import numpy as np
import pytest

from tests import _mxfp6 as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "cpp", "test_mxfp6")
N = M.TILE + 96 + 17  # a whole tile of block pairs, an odd count of further blocks, a ragged tail with n % 4 = 1
SEED, FIRST = 0x0123456789ABCDEF, 64


def _exe():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fmi_amd", "cpp")], check=True)
    return EXE


@pytest.mark.parametrize("kind", M.KINDS)
def test_cpp_host_pack_widen_narrow_and_host_sr(tmp_path, kind):
    """No device: narrow on every grid value, tie and neighbour and on random values within range, widen of the 64 codes,
    fp6_pack of the codes, and the host stochastic-rounding quantization, against files written from tests/_mxfp6.py."""
    rng = np.random.default_rng(4)
    b = np.concatenate([M.exhaustive_values(kind), ((rng.random(4001) * 2 - 1) * M.MAX[kind]).astype(np.float32)]).astype(np.float32)
    b.tofile(tmp_path / "src.f32")
    out = [str(tmp_path / k) for k in ("codes", "table", "packed", "sr", "sr_scales")]
    run = subprocess.run([_exe(), "host", kind, str(b.size), str(tmp_path / "src.f32")] + out, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    want = M.narrow(b, kind)
    assert np.array_equal(np.fromfile(out[0], np.uint8), want)
    assert np.array_equal(np.fromfile(out[1], np.float32).view(np.uint32), M.TABLE[kind].view(np.uint32))
    assert np.array_equal(np.fromfile(out[2], np.uint8), M.pack(want))
    sr, sr_sc = M.quant_sr(b, kind, SEED, FIRST)
    assert np.array_equal(np.fromfile(out[3], np.uint8), M.pack(sr)) and np.array_equal(np.fromfile(out[4], np.uint8), sr_sc)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", M.KINDS)
def test_cpp_reduce_tree_mxfp6(tmp_path, kind):
    """One fused call per output form, the stochastic-rounding call, and the fallback route (P = 1)."""
    n = N
    for P, cases in ((5, ((0, "allreduce", 0, "sum", "f32"), (2, "reduce_ltr", 5, "avg", "same"), (1, "reduce", 0, "sum", "same"),
                          (0, "allreduce", 0, "sum", "sr"))),
                     (1, ((0, "allreduce", 0, "sum", "same"),))):
        xs, es = M.random_inputs(n, P, 7, 112, 142)
        np.concatenate([M.pack(x) for x in xs]).tofile(tmp_path / "in.u8")
        np.concatenate(es).tofile(tmp_path / "scales.u8")
        for alg, family, op, opname, out in cases:
            res, rsc = tmp_path / f"res_{P}_{alg}_{out}", tmp_path / f"rsc_{P}_{alg}_{out}"
            arg = f"sr:{SEED}:{FIRST}" if out == "sr" else out
            run = subprocess.run([_exe(), "reduce", kind, str(op), str(alg), arg, str(P), str(n), str(tmp_path / "in.u8"),
                                  str(tmp_path / "scales.u8"), str(res), str(rsc)], capture_output=True, text=True, timeout=120)
            assert run.returncode == 0, run.stderr[-2000:]
            what = f"C++ {kind} {family} {opname} {out} P={P}"
            if out == "f32":
                M.assert_mx(np.fromfile(res, np.float32), None, M.values(family, kind, xs, es, opname), None, out, what)
                continue
            want, want_sc = M.expected_sr(family, kind, xs, es, SEED, FIRST, opname) if out == "sr" else M.expected(family, kind, xs, es, opname)
            raw = np.fromfile(res, np.uint8)
            assert raw.size == M.nbytes(n)
            M.assert_mx(M.unpack(raw, n), np.fromfile(rsc, np.uint8), want, want_sc, "same", what)
            assert np.array_equal(raw, M.pack(want)), f"{what}: the last byte's spare bits are not 0"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", M.KINDS)
def test_cpp_quantize_round_trip(tmp_path, kind):
    """float -> MXFP6 -> float through Dev::mx_quantize and Dev::mx_dequantize."""
    n = N
    xs, es = M.random_inputs(n, 1, 9)
    S = (M.dequant(xs[0], es[0], kind) * np.float32(1.37)).astype(np.float32)
    S.tofile(tmp_path / "src.f32")
    q, sc, back = tmp_path / "q", tmp_path / "sc", tmp_path / "back"
    run = subprocess.run([_exe(), "quantize", kind, str(n), str(tmp_path / "src.f32"), str(q), str(sc), str(back)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    want, want_sc = M.quant(S, kind)
    raw = np.fromfile(q, np.uint8)
    assert np.array_equal(raw, M.pack(want))
    M.assert_mx(M.unpack(raw, n), np.fromfile(sc, np.uint8), want, want_sc, "same", "C++ quantize")
    M.assert_mx(np.fromfile(back, np.float32), None, M.dequant(want, want_sc, kind), None, "f32", "C++ dequantize")
