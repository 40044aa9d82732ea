"""One process of tests/test_gpu_fp8_scaled.py::test_torch_glue (torch has to be loaded before the library):

    python -m tests._fp8_scaled_torch_worker

fmi_amd.collectives.HipEngine.reduce_tree_scaled on torch.float8_e4m3fn / float8_e5m2 device tensors with float32 scale
tensors, 5 peers of n = 3 * 4096 + 7, both outputs, against the definition (tests/_fp8_scaled.py). Prints
"fp8 scaled torch glue ok" on success."""
import numpy as np
import torch

from fmi_amd import Alg
from fmi_amd.collectives import HipEngine
from tests import _fp8 as F
from tests import _fp8_scaled as FS

TORCH = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def main():
    eng = HipEngine(0)
    n, P = 3 * 4096 + 7, 5
    s = FS.scales(P)
    for kind in F.KINDS:
        xs = [F.synthetic(kind, n, seed=23, peer=p) for p in range(P)]
        ts = [torch.from_numpy(x.copy()).view(TORCH[kind]).to(eng.device) for x in xs]
        sc = torch.from_numpy(s.copy()).to(eng.device)
        t = torch.tensor([float(FS.T_OUT)], dtype=torch.float32, device=eng.device)
        for out, alg, family in (("f32", Alg.ALLREDUCE, "allreduce"), ("same", Alg.REDUCE_LTR, "reduce_ltr")):
            o = torch.empty(n, dtype=torch.float32 if out == "f32" else TORCH[kind], device=eng.device)
            amax = torch.zeros(1, dtype=torch.float32, device=eng.device)
            eng.reduce_tree_scaled(alg, o, ts, sc, t, amax)
            torch.cuda.synchronize()
            want, want_amax, _ = FS.expected_scaled(family, kind, xs, s, FS.T_OUT, out)
            got = o.cpu().numpy() if out == "f32" else o.cpu().view(torch.uint8).numpy()
            FS.assert_out(got, want, kind, out, f"torch glue {kind} {family}")
            FS.assert_amax(int(amax.cpu().numpy().view(np.uint32)[0]), want_amax, f"torch glue {kind} {family}")
        try:
            eng.reduce_tree_scaled(Alg.ALLREDUCE, torch.empty(n, dtype=torch.bfloat16, device=eng.device), ts, sc)
        except ValueError:
            pass
        else:
            raise AssertionError("a bfloat16 output was accepted")
    print("fp8 scaled torch glue ok", flush=True)


if __name__ == "__main__":
    main()
