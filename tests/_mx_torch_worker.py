"""One process of tests/test_gpu_mx.py::test_torch_glue (torch has to be loaded before the library):

    python -m tests._mx_torch_worker

fmi_amd.collectives.HipEngine.reduce_tree_mx on torch.float8_e4m3fn / float8_e5m2 device tensors with float8_e8m0fnu
scale tensors, 5 peers of n = 4096 + 96 + 17, both outputs, against the definition (tests/_mx.py); the 8-bit result is
read back through torch's own float8 and e8m0 conversions as well. Prints "mx torch glue ok" on success."""
import numpy as np
import torch

from fmi_amd import Alg, Op
from fmi_amd.collectives import HipEngine
from tests import _fp8 as F
from tests import _mx as MX

TORCH = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def main():
    eng = HipEngine(0)
    n, P = 4096 + 96 + 17, 5
    for kind in F.KINDS:
        xs, es = MX.random_inputs(kind, n, P, seed=23, finite=True)
        ts = [torch.from_numpy(x.copy()).view(TORCH[kind]).to(eng.device) for x in xs]
        scs = [torch.from_numpy(e.copy()).view(torch.float8_e8m0fnu).to(eng.device) for e in es]
        for out, op, alg, family in (("f32", "sum", Alg.ALLREDUCE, "allreduce"), ("same", "avg", Alg.REDUCE_LTR, "reduce_ltr")):
            o = torch.empty(n, dtype=torch.float32 if out == "f32" else TORCH[kind], device=eng.device)
            osc = None if out == "f32" else torch.empty(MX.blocks(n), dtype=torch.float8_e8m0fnu, device=eng.device)
            eng.reduce_tree_mx(Op.SUM if op == "sum" else Op.AVG, alg, o, osc, ts, scs)
            torch.cuda.synchronize()
            want, want_sc = MX.expected_mx(family, kind, xs, es, op, out)
            if out == "f32":
                MX.assert_mx(o.cpu().numpy(), None, want, None, kind, out, f"torch glue {kind} {family}")
                continue
            got, got_sc = o.cpu().view(torch.uint8).numpy(), osc.cpu().view(torch.uint8).numpy()
            MX.assert_mx(got, got_sc, want, want_sc, kind, out, f"torch glue {kind} {family}")
            # the round trip through torch's own decoding: elements times scales equals the definition's dequant
            back = o.cpu().to(torch.float32) * osc.cpu().to(torch.float32).repeat_interleave(32)[:n]
            assert np.array_equal(back.numpy().view(np.uint32), MX.dequant(want, want_sc, kind).view(np.uint32))
        for bad, exc in ((dict(out=torch.empty(n, dtype=torch.bfloat16, device=eng.device)), ValueError),
                         (dict(osc=None), ValueError),
                         (dict(osc=torch.empty(MX.blocks(n) + 1, dtype=torch.uint8, device=eng.device)), ValueError)):
            o = bad.get("out", torch.empty(n, dtype=TORCH[kind], device=eng.device))
            osc = bad.get("osc", torch.empty(MX.blocks(n), dtype=torch.uint8, device=eng.device))
            try:
                eng.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, o, osc, ts, scs)
            except exc:
                pass
            else:
                raise AssertionError(f"accepted: {bad}")
    print("mx torch glue ok", flush=True)


if __name__ == "__main__":
    main()
