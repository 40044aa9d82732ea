"""One process of tests/test_gpu_fp8.py::test_torch_glue (torch has to be loaded before the library):

    python -m tests._fp8_torch_worker

fmi_amd.collectives' pair combine and 5-peer f32-accumulating reduce_tree on torch.float8_e4m3fn device tensors of
n = 8245 against the ctypes path (fmi_amd.reduce_pair / reduce_tree on Buckets of the same bytes) and the definition
(tests/_fp8.py). Prints "fp8 torch glue ok" on success."""
import numpy as np
import torch

import fmi_amd
from fmi_amd import Alg, Bucket, DType, Op
from fmi_amd.collectives import HipEngine
from tests import _fp8 as F


def main():
    eng = HipEngine(0)
    n, P, kind = 8245, 5, "e4m3"
    xs = [F.synthetic(kind, n, seed=23, peer=p) for p in range(P)]
    ts = [torch.from_numpy(x.copy()).view(torch.float8_e4m3fn).to(eng.device) for x in xs]
    bs = []
    for x in xs:
        b = Bucket(n, DType.F8E4M3)
        b.upload(x)
        bs.append(b)
    back = lambda t: t.cpu().view(torch.uint8).numpy()  # noqa: E731
    # P-way, f32 accumulation
    out_t, out_b = torch.empty_like(ts[0]), Bucket(n, DType.F8E4M3)
    eng.reduce_tree(Op.SUM, Alg.ALLREDUCE, out_t, ts, rank=2, accumulate_f32=True)
    fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, out_b, bs, rank=2, accumulate_f32=True)
    torch.cuda.synchronize()
    fmi_amd.sync()
    assert np.array_equal(back(out_t), out_b.numpy()), "torch glue reduce_tree differs from the ctypes path"
    F.assert_bits(back(out_t), F.expected_acc("allreduce", kind, "sum", xs)[2], kind, "torch glue reduce_tree")
    # pairwise
    eng.reduce_pair(Op.SUM, ts[0], ts[1])
    fmi_amd.reduce_pair(Op.SUM, bs[0], bs[1])
    torch.cuda.synchronize()
    fmi_amd.sync()
    assert np.array_equal(back(ts[0]), bs[0].numpy()), "torch glue reduce_pair differs from the ctypes path"
    F.assert_bits(back(ts[0]), F.combine("sum", xs[0], xs[1], kind), kind, "torch glue reduce_pair")
    assert np.array_equal(back(ts[1]), xs[1]), "src untouched"
    print("fp8 torch glue ok", flush=True)


if __name__ == "__main__":
    main()
