"""One process of tests/test_gpu_half.py::test_torch_glue_pair_combine (torch has to be loaded before the library):

    python -m tests._half_torch_worker

fmi_amd.collectives' pair combine on torch.bfloat16 / torch.float16 device tensors of n = 8205 against torch CPU's
a + b on the same bits. Prints "half torch glue ok" on success."""
import numpy as np
import torch

from fmi_amd import Op
from fmi_amd.collectives import HipEngine
from tests import _half as H


def main():
    eng = HipEngine(0)
    n = 8205
    for kind, tdt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        a_bits, b_bits = H.inputs(kind, n, seed=21, peer=0), H.inputs(kind, n, seed=21, peer=1)
        a = torch.from_numpy(a_bits.view(np.int16).copy()).view(tdt)
        b = torch.from_numpy(b_bits.view(np.int16).copy()).view(tdt)
        want = (a + b).view(torch.int16).numpy().view(np.uint16)
        da, db = a.to(eng.device), b.to(eng.device)
        eng.reduce_pair(Op.SUM, da, db)
        torch.cuda.synchronize()
        H.assert_bits(da.cpu().view(torch.int16).numpy().view(np.uint16), want, kind, "sum", f"torch glue {kind}")
        H.assert_bits(db.cpu().view(torch.int16).numpy().view(np.uint16), b_bits, kind, "max", "src untouched")
    print("half torch glue ok", flush=True)


if __name__ == "__main__":
    main()
