"""One process of tests/test_gpu_mxfp6.py::test_torch_glue (torch has to be loaded before the library):

    python -m tests._mxfp6_torch_worker

fmi_amd.collectives.HipEngine.reduce_tree_mx on torch.uint8 device tensors of packed FP6 bytes with the keywords dtype=
and n= (torch has no 6-bit dtype) and float8_e8m0fnu scale tensors, 5 peers of n = 16384 + 96 + 18, both types, the f32
output, the FP6 output and stochastic rounding, against the definition (tests/_mxfp6.py). Prints "mxfp6 torch glue ok" on
success."""
import numpy as np
import torch

from fmi_amd import Alg, DType, Op
from fmi_amd.collectives import HipEngine
from tests import _mx as MX
from tests import _mxfp6 as M


def main():
    eng = HipEngine(0)
    n, P, seed = M.TILE + 96 + 18, 5, 0x0123456789ABCDEF
    nbytes = M.nbytes(n)
    for kind, dt in (("e2m3", DType.F6E2M3), ("e3m2", DType.F6E3M2)):
        xs, es = M.random_inputs(n, P, 23, 112, 142)
        ts = [torch.from_numpy(M.pack(x)).to(eng.device) for x in xs]
        scs = [torch.from_numpy(e.copy()).view(torch.float8_e8m0fnu).to(eng.device) for e in es]
        word = torch.from_numpy(np.array([seed], np.uint64).view(np.int64)).to(eng.device)
        for out, op, alg, family in (("f32", "sum", Alg.ALLREDUCE, "allreduce"), ("same", "avg", Alg.REDUCE_LTR, "reduce_ltr"),
                                     ("sr", "sum", Alg.ALLREDUCE, "allreduce")):
            if out == "f32":
                o, osc = torch.empty(n, dtype=torch.float32, device=eng.device), None
            else:
                o = torch.empty(nbytes, dtype=torch.uint8, device=eng.device)
                osc = torch.empty(MX.blocks(n), dtype=torch.float8_e8m0fnu, device=eng.device)
            kw = {"seed": word, "first": 64} if out == "sr" else {}
            eng.reduce_tree_mx(Op.SUM if op == "sum" else Op.AVG, alg, o, osc, ts, scs, dtype=dt, n=n, **kw)
            torch.cuda.synchronize()
            if out == "f32":
                M.assert_mx(o.cpu().numpy(), None, M.values(family, kind, xs, es, op), None, out, f"torch glue {kind} {family}")
                continue
            want, want_sc = M.expected_sr(family, kind, xs, es, seed, 64, op) if out == "sr" else M.expected(family, kind, xs, es, op)
            raw = o.cpu().numpy()
            M.assert_mx(M.unpack(raw, n), osc.view(torch.uint8).cpu().numpy(), want, want_sc, "same", f"torch glue {kind} {family} {out}")
            assert np.array_equal(raw, M.pack(want))
        for o, kw in ((torch.empty(n - 1, dtype=torch.float32, device=eng.device), {"dtype": dt, "n": n}),       # not n values
                      (torch.empty(nbytes, dtype=torch.uint8, device=eng.device), {"dtype": dt, "n": n}),         # no out_scales
                      (torch.empty(n, dtype=torch.float32, device=eng.device), {"dtype": dt}),                    # no n
                      (torch.empty(n, dtype=torch.float32, device=eng.device), {"dtype": dt, "n": n + 1}),        # not the bytes of n + 1
                      (torch.empty(n, dtype=torch.float32, device=eng.device), {"n": n})):                        # n without the type
            try:
                eng.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, o, None, ts, scs, **kw)
            except (ValueError, TypeError):
                pass
            else:
                raise AssertionError(f"accepted: {o.dtype} x {o.numel()}, {kw}")
    print("mxfp6 torch glue ok", flush=True)


if __name__ == "__main__":
    main()
