"""One rank of a 2-rank PROC-transport communicator on 8-bit float buckets, run as its own process by
tests/test_gpu_fp8.py::test_comm_proc_transport:

    python -m tests._fp8_proc_worker <uid hex> <nranks> <rank> <out.npz>

An f32-accumulating allreduce (SUM) and a plain allreduce (MAX) per format on the buckets the parent regenerates; saves
what this rank received. The parent compares each array with the oracle; this process only computes."""
import sys

import numpy as np

import fmi_amd
from fmi_amd import Bucket, DType, Op
from fmi_amd.comm import Comm, Path
from tests import _fp8 as F

N_ELEMS, SEED = 3 * 4096 + 7, 83
DT = {"e4m3": DType.F8E4M3, "e5m2": DType.F8E5M2}


def main():
    uid, N, r, path = bytes.fromhex(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    fmi_amd.init(0)
    c = Comm(uid, N, r)
    out = {}
    for kind in F.KINDS:
        s = Bucket(N_ELEMS, DT[kind])
        s.upload(F.cancel_inputs(kind, N_ELEMS, N, SEED)[r])
        acc, mx = Bucket(N_ELEMS, DT[kind]), Bucket(N_ELEMS, DT[kind])
        c.allreduce(Op.SUM, s, acc, path=Path.TREE, accumulate_f32=True)
        c.allreduce(Op.MAX, s, mx)
        fmi_amd.sync()
        out[f"{kind}_acc_sum"], out[f"{kind}_max"] = acc.numpy(), mx.numpy()
    c.destroy()
    np.savez(path, **out)


if __name__ == "__main__":
    main()
