"""One process of tests/test_gpu_mxfp4.py::test_torch_glue (torch has to be loaded before the library):

    python -m tests._mxfp4_torch_worker

fmi_amd.collectives.HipEngine.reduce_tree_mx on torch.float4_e2m1fn_x2 device tensors (two elements per tensor element:
n = 2 * numel) with float8_e8m0fnu scale tensors, 5 peers of n = 8192 + 96 + 18, both outputs, against the definition
(tests/_mxfp4.py). Prints "mxfp4 torch glue ok" on success."""
import torch

from fmi_amd import Alg, Op
from fmi_amd.collectives import HipEngine
from tests import _mx as MX
from tests import _mxfp4 as M


def main():
    eng = HipEngine(0)
    n, P = 8192 + 96 + 18, 5
    xs, es = M.random_inputs(n, P, 23, 112, 142)
    ts = [torch.from_numpy(M.pack(x)).view(torch.float4_e2m1fn_x2).to(eng.device) for x in xs]
    scs = [torch.from_numpy(e.copy()).view(torch.float8_e8m0fnu).to(eng.device) for e in es]
    assert ts[0].numel() == n // 2
    for out, op, alg, family in (("f32", "sum", Alg.ALLREDUCE, "allreduce"), ("same", "avg", Alg.REDUCE_LTR, "reduce_ltr")):
        if out == "f32":
            o, osc = torch.empty(n, dtype=torch.float32, device=eng.device), None
        else:
            o = torch.empty(n // 2, dtype=torch.uint8, device=eng.device).view(torch.float4_e2m1fn_x2)
            osc = torch.empty(MX.blocks(n), dtype=torch.float8_e8m0fnu, device=eng.device)
        eng.reduce_tree_mx(Op.SUM if op == "sum" else Op.AVG, alg, o, osc, ts, scs)
        torch.cuda.synchronize()
        want, want_sc = M.expected(family, xs, es, op, out)
        if out == "f32":
            M.assert_mx(o.cpu().numpy(), None, want, None, out, f"torch glue {family}")
        else:
            got = M.unpack(o.view(torch.uint8).cpu().numpy(), n)
            M.assert_mx(got, osc.view(torch.uint8).cpu().numpy(), want, want_sc, out, f"torch glue {family}")
    for o, osc in ((torch.empty(n // 2, dtype=torch.float32, device=eng.device), None),                       # n / 2 values
                   (torch.empty(n // 2, dtype=torch.uint8, device=eng.device).view(torch.float4_e2m1fn_x2), None),
                   (torch.empty(n, dtype=torch.float32, device=eng.device), torch.empty(MX.blocks(n) + 1, dtype=torch.uint8, device=eng.device))):
        try:
            eng.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, o, osc, ts, scs)
        except ValueError:
            pass
        else:
            raise AssertionError(f"accepted: {o.dtype} x {o.numel()}, scales {osc}")
    print("mxfp4 torch glue ok", flush=True)


if __name__ == "__main__":
    main()
