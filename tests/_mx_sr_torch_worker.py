"""One process of tests/test_gpu_mx_sr.py::test_torch_glue (torch has to be loaded before the library):

    python -m tests._mx_sr_torch_worker

fmi_amd.collectives.HipEngine.reduce_tree_mx(seed=...) on float8_e4m3fn, float8_e5m2 and float4_e2m1fn_x2 device tensors
with float8_e8m0fnu scale tensors, 5 peers, the seed a one-element int64 device tensor whose bits are used as they are
(a negative value is a seed above 2^63), against the definition (tests/_mx_sr.py). Prints "mx sr torch glue ok" per
element type."""
import numpy as np
import torch

from fmi_amd import Alg, Op
from fmi_amd.collectives import HipEngine
from tests import _mx as MX
from tests import _mx_sr as SR

TORCH = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2, "e2m1": torch.float4_e2m1fn_x2}


def main():
    eng = HipEngine(0)
    n, P, first = 8192 + 96 + 18, 5, 64
    seed = 2 ** 64 - 12345
    word = torch.tensor([seed - 2 ** 64], dtype=torch.int64, device=eng.device)
    for kind in SR.KINDS:
        xs, es = SR.visible_inputs(kind, n, P)
        ts = [torch.from_numpy(SR.element_bytes(x, kind).copy()).view(TORCH[kind]).to(eng.device) for x in xs]
        scs = [torch.from_numpy(e.copy()).view(torch.float8_e8m0fnu).to(eng.device) for e in es]
        o = torch.empty(ts[0].numel(), dtype=torch.uint8, device=eng.device).view(TORCH[kind])
        osc = torch.empty(MX.blocks(n), dtype=torch.float8_e8m0fnu, device=eng.device)
        eng.reduce_tree_mx(Op.AVG, Alg.REDUCE_LTR, o, osc, ts, scs, seed=word, first=first)
        torch.cuda.synchronize()
        want, want_sc = SR.expected_sr("reduce_ltr", kind, xs, es, seed, first, "avg")
        got = SR.codes_of(o.view(torch.uint8).cpu().numpy(), kind, n)
        assert np.array_equal(osc.view(torch.uint8).cpu().numpy(), want_sc), f"torch glue {kind}: scale bytes"
        assert np.array_equal(got, want), f"torch glue {kind}: {(got != want).sum()} codes differ"
        for bad_seed, bad_out in ((word.to(torch.int32), o), (torch.zeros(2, dtype=torch.int64, device=eng.device), o), (word.cpu(), o),
                                  (word, torch.empty(n, dtype=torch.float32, device=eng.device))):
            try:
                eng.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, bad_out, osc, ts, scs, seed=bad_seed)
            except ValueError:
                pass
            else:
                raise AssertionError(f"accepted: seed {bad_seed.dtype} x {bad_seed.numel()} on {bad_seed.device}, out {bad_out.dtype}")
        print("mx sr torch glue ok", kind, flush=True)


if __name__ == "__main__":
    main()
