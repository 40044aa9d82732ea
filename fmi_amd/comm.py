"""Python handle over the C-ABI communicator (include/fmi_dev.h, "sharded device collectives").

`Comm` wraps fmi_comm_*: sharded allreduce / reduce / scan of device buckets across ranks (one rank per
GPU over RCCL, ranks as threads of one process over the LOCAL transport, or processes of one node over
PROC), with the combine done by the
fused kernels in the reference's evaluation order (reference src/comm/PeerToPeer.cpp). Buffers are
`fmi_amd.Bucket`s or raw device pointers.
"""
from __future__ import annotations

import ctypes
import enum
import os
from typing import Optional

from . import _lib
import numpy as np

from ._lib import Timeout  # noqa: F401 - FMI_ERR_TIMEOUT, the reference's FMI::Utils::Timeout

from .device import (Alg, Bucket, DType, Op, _f32_word, _mx_elements, _mx_scales, _sptr, _sr_seed, acc_dtype, dtype_of, itemsize_of,
                     refuse_fp4)

ID_BYTES = 128


class Transport(enum.IntEnum):
    RCCL = 0
    LOCAL = 1
    PROC = 2  # ranks are processes of one node (same or different GPUs): shared-memory staging + HIP IPC windows


class Path(enum.IntEnum):
    TREE = 0  # all-to-all + fused kernel in the reference's order + all-gather (bit-exact)
    RCCL = 1  # RCCL reduce-scatter + all-gather (RCCL's order)
    DIRECT = 2  # fused kernel reading every rank's window over xGMI + direct gather (bit-exact, windows only)


def unique_id(transport: Transport = Transport.RCCL) -> bytes:
    buf = ctypes.create_string_buffer(ID_BYTES)
    _lib.call("fmi_comm_unique_id", int(transport), buf, ID_BYTES)
    return buf.raw


VISIBILITY_ENV = ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "GPU_MAX_HW_QUEUES")


def runtime_info() -> dict:
    """What a multi-GPU run needs to be diagnosable from one line: the librccl the RCCL transport runs on
    (fmi_comm_rccl_info: ncclGetVersion and the real path of the mapped object) and the device-visibility /
    hardware-queue environment of this process. Never raises: a failure is reported in the dict."""
    info = {k: os.environ.get(k) for k in VISIBILITY_ENV}
    try:
        v = ctypes.c_int(0)
        path = ctypes.create_string_buffer(4096)
        _lib.call("fmi_comm_rccl_info", ctypes.byref(v), path, len(path))
        info["rccl_version"] = v.value
        info["rccl_path"] = path.value.decode(errors="replace")
    except Exception as e:  # reported, never raised: this runs on error paths
        info["rccl_error"] = f"{type(e).__name__}: {e}"
    return info


def _p(x) -> Optional[int]:
    if x is None:
        return None
    return x.ptr if isinstance(x, Bucket) else int(x)


class Comm:
    def __init__(self, uid: bytes, nranks: int, rank: int, timeout_s: Optional[float] = None):
        """timeout_s: how long any wait for the peers may last (init rendezvous, barriers, sync); None = the
        library default (FMI_COMM_TIMEOUT_S, else 300 s). Expiry raises Timeout and aborts the communicator."""
        if len(uid) != ID_BYTES:
            raise ValueError("communicator id must be 128 bytes")
        h = ctypes.c_void_p()
        self._id = ctypes.create_string_buffer(uid, ID_BYTES)
        _lib.call("fmi_comm_init_timeout", ctypes.byref(h), self._id, nranks, rank, float(timeout_s or 0.0))
        self.handle = h.value
        self.nranks = nranks
        self.rank = rank

    def destroy(self) -> None:
        if self.handle:
            _lib.call("fmi_comm_destroy", self.handle)
            self.handle = None

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.load().fmi_comm_destroy(self.handle)
        except Exception:
            pass

    def sync(self, stream=None) -> None:
        """Wait for the collectives enqueued on `stream` (None = library stream) within the communicator's
        timeout; raises Timeout (the communicator is then aborted) or FmiError on a transport error."""
        _lib.call("fmi_comm_sync", self.handle, _sptr(stream))

    def query(self) -> dict:
        """What the transport reports about this rank: RCCL's own rank count, rank and device
        (ncclCommCount / ncclCommUserRank / ncclCommCuDevice); the communicator's for LOCAL / PROC."""
        cnt, rk, dev = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.call("fmi_comm_query", self.handle, ctypes.byref(cnt), ctypes.byref(rk), ctypes.byref(dev))
        return {"count": cnt.value, "rank": rk.value, "device": dev.value}

    def timing(self, enable: bool) -> None:
        """Record an event pair around every shard-kernel launch of the collectives (fmi_comm_timing)."""
        _lib.call("fmi_comm_timing", self.handle, 1 if enable else 0)

    def timing_read(self):
        """(total shard-kernel ms, launches) since timing was enabled or last read."""
        ms, k = ctypes.c_float(), ctypes.c_int()
        _lib.call("fmi_comm_timing_read", self.handle, ctypes.byref(ms), ctypes.byref(k))
        return float(ms.value), int(k.value)

    def allreduce(self, op: Op, send: Bucket, recv: Bucket, ordered: bool = False, path: Path = Path.TREE,
                  stream=None, accumulate_f32: bool = False) -> None:
        """accumulate_f32 (F16 / BF16 / F8E4M3 / F8E5M2 buckets, here and in allreduce_host / reduce / scan): every
        rank's shard is reduced on f32 values and rounded to the storage type once (FMI_ACC_F32); the wire keeps the
        storage type. Every rank passes the same value. Path.RCCL has its own order and rounding and refuses it, as it
        refuses the 8-bit float dtypes altogether.
        Op.AVG (float buckets; here, in allreduce_host and in reduce): the mean over the ranks, the sum's value times
        the rounded reciprocal of the rank count before the shard's one store (FMI_OP_AVG); Path.RCCL reduce-scatters
        with SUM and scales its shard. scan and reduce(sendbuf_partials=True) refuse it."""
        refuse_fp4("allreduce", send, recv)
        alg = Alg.REDUCE_LTR if ordered else Alg.ALLREDUCE
        arg = acc_dtype(send.dtype, accumulate_f32)
        _lib.call("fmi_comm_allreduce", self.handle, int(op), arg, int(alg), int(path), _p(send), _p(recv), send.n,
                  _sptr(stream))

    def allreduce_scaled(self, send: Bucket, in_scale: Bucket, recv: Bucket, out_scale: Optional[Bucket] = None,
                         amax: Optional[Bucket] = None, ordered: bool = False, stream=None) -> None:
        """The sharded allreduce of scaled F8E4M3 / F8E5M2 buckets (fmi_comm_allreduce_scaled, path TREE): rank r's
        `send` times its own `in_scale` in f32, the f32 sum over the ranks in the reference's order, times `out_scale`,
        into `recv` (the inputs' dtype or F32) on every rank; `amax` ends as the largest |sum| over the whole bucket,
        folded into what it held, the same on every rank. The wire carries the 8-bit bytes and one scale per rank.
        in_scale / out_scale / amax are one-element F32 buckets; out_scale holds the same value on every rank."""
        if send.dtype not in (DType.F8E4M3, DType.F8E5M2):
            raise ValueError(f"allreduce_scaled needs an F8E4M3 or F8E5M2 send bucket, got {DType(send.dtype).name}")
        if recv.n != send.n or recv.dtype not in (send.dtype, DType.F32):
            raise ValueError("allreduce_scaled: `recv` must hold send's length in its dtype or in F32")
        alg = Alg.REDUCE_LTR if ordered else Alg.ALLREDUCE
        _lib.call("fmi_comm_allreduce_scaled", self.handle, int(Op.SUM), int(send.dtype), int(alg), int(recv.dtype),
                  _p(send), _f32_word(in_scale, "in_scale"), _p(recv), _f32_word(out_scale, "out_scale"),
                  _f32_word(amax, "amax"), send.n, _sptr(stream))

    def allreduce_mx(self, op: Op, send: Bucket, send_scales: Bucket, recv: Bucket, recv_scales: Optional[Bucket] = None,
                     ordered: bool = False, stream=None, seed: Optional[Bucket] = None, first: int = 0) -> None:
        """The sharded allreduce of MX buckets (fmi_comm_allreduce_mx, path TREE): the sum (Op.SUM) or mean (Op.AVG)
        over the ranks of `send` under its block scales `send_scales` (F8E8M0, ceil(n / 32) bytes), in the reference's
        order, into `recv` on every rank: an F32 bucket (recv_scales None), or a bucket of send's dtype requantized
        block by block with its scale bytes in `recv_scales`. The wire carries the element bytes and the scale bytes.
        F4E2M1 buckets (MXFP4) travel packed, at half the element bytes, F6E2M3 / F6E3M2 buckets (MXFP6) at three quarters.
        seed: a U64 bucket of one element selects stochastic rounding (fmi_comm_allreduce_mx_sr; `recv` of send's dtype):
        every rank holds the same value in it and passes the same `first`, a multiple of 32, and every rank's result is
        device.reduce_tree_mx's over the ranks' buckets at that (seed, first)."""
        dtype = _mx_elements("allreduce_mx", "send bucket", send)
        if recv.n != send.n or recv.dtype not in (dtype, DType.F32):
            raise ValueError("allreduce_mx: `recv` must hold send's length in its dtype or in F32")
        if recv.dtype != DType.F32 and recv_scales is None:
            raise ValueError("allreduce_mx: recv_scales is missing: only an F32 output has no scale bytes")
        alg = Alg.REDUCE_LTR if ordered else Alg.ALLREDUCE
        if seed is not None:
            word = _sr_seed("allreduce_mx", seed, recv, first)
            _lib.call("fmi_comm_allreduce_mx_sr", self.handle, int(op), int(dtype), int(alg), _p(send),
                      _mx_scales(send_scales, "send_scales", send.n), _p(recv), _mx_scales(recv_scales, "recv_scales", send.n),
                      send.n, word, int(first), _sptr(stream))
            return
        _lib.call("fmi_comm_allreduce_mx", self.handle, int(op), int(dtype), int(alg), int(recv.dtype), _p(send),
                  _mx_scales(send_scales, "send_scales", send.n), _p(recv),
                  None if recv_scales is None else _mx_scales(recv_scales, "recv_scales", send.n), send.n, _sptr(stream))

    def window(self, n: int, dtype) -> Bucket:
        """A symmetric window bucket for Path.DIRECT (collective: every rank, same n and dtype). Release it
        with window_free (collective) or with the communicator."""
        nbytes = int(n) * itemsize_of(dtype)
        p = ctypes.c_void_p()
        _lib.call("fmi_comm_window_alloc", self.handle, nbytes, ctypes.byref(p))
        return Bucket(n, dtype, ptr=p.value)

    def window_free(self, b: Bucket) -> None:
        _lib.call("fmi_comm_window_free", self.handle, b.ptr)
        b.ptr = 0

    def allreduce_host(self, op: Op, send: np.ndarray, recv: np.ndarray, ordered: bool = False,
                       path: Path = Path.TREE, chunk: int = 0, accumulate_f32: bool = False, dtype=None) -> None:
        """Allreduce of HOST arrays (channel recv buffers, config C5), streamed through the GPU in
        `chunk`-element pieces (0 = FMI_TUNE_HOST_CHUNK). Page-locked arrays (PinnedArray.array) take the
        DMA path. Blocking: `recv` holds the result on return. `dtype`: the element type where the arrays carry raw
        bits (DType.BF16 over np.uint16); None = the arrays' own."""
        if send.dtype != recv.dtype or send.size != recv.size:
            raise ValueError("allreduce_host: arrays must share dtype and size")
        if not (send.flags.c_contiguous and recv.flags.c_contiguous):
            raise ValueError("allreduce_host: arrays must be contiguous")
        if dtype is not None and DType(dtype) in (DType.F4E2M1, DType.F6E2M3, DType.F6E3M2):
            raise ValueError(f"allreduce_host: {DType(dtype).name} is valid only in the MX calls")
        alg = Alg.REDUCE_LTR if ordered else Alg.ALLREDUCE
        arg = acc_dtype(dtype_of(send) if dtype is None else dtype, accumulate_f32)
        _lib.call("fmi_comm_allreduce_host", self.handle, int(op), arg, int(alg), int(path),
                  send.ctypes.data, recv.ctypes.data, send.size, int(chunk))

    def reduce(self, op: Op, send: Bucket, recv: Optional[Bucket], root: int, ordered: bool = False,
               stream=None, sendbuf_partials: bool = False, accumulate_f32: bool = False) -> None:
        """sendbuf_partials=True: `send` ends as the reference leaves peer `rank`'s sendbuf (the partial it
        forwarded up the binomial tree, reference src/comm/PeerToPeer.cpp:72) — fmi_comm_reduce_sendbuf."""
        alg = Alg.REDUCE_LTR if ordered else Alg.REDUCE
        fn = "fmi_comm_reduce_sendbuf" if sendbuf_partials else "fmi_comm_reduce"
        refuse_fp4("reduce", send, recv)
        arg = acc_dtype(send.dtype, accumulate_f32)
        _lib.call(fn, self.handle, int(op), arg, int(alg), _p(send), _p(recv), send.n, root, _sptr(stream))

    def scan(self, op: Op, send: Bucket, recv: Bucket, ordered: bool = False, stream=None,
             accumulate_f32: bool = False) -> None:
        refuse_fp4("scan", send, recv)
        alg = Alg.SCAN_LTR if ordered else Alg.SCAN
        arg = acc_dtype(send.dtype, accumulate_f32)
        _lib.call("fmi_comm_scan", self.handle, int(op), arg, int(alg), _p(send), _p(recv), send.n, _sptr(stream))

    def bcast(self, buf: Bucket, root: int, stream=None) -> None:
        _lib.call("fmi_comm_bcast", self.handle, _p(buf), buf.nbytes, root, _sptr(stream))

    def gather(self, send: Bucket, recv: Optional[Bucket], root: int, stream=None) -> None:
        _lib.call("fmi_comm_gather", self.handle, _p(send), _p(recv), send.nbytes, root, _sptr(stream))

    def scatter(self, send: Optional[Bucket], recv: Bucket, root: int, stream=None) -> None:
        _lib.call("fmi_comm_scatter", self.handle, _p(send), _p(recv), recv.nbytes, root, _sptr(stream))

    def send(self, buf: Bucket, peer: int, stream=None) -> None:
        _lib.call("fmi_comm_send", self.handle, _p(buf), buf.nbytes, peer, _sptr(stream))

    def recv(self, buf: Bucket, peer: int, stream=None) -> None:
        _lib.call("fmi_comm_recv", self.handle, _p(buf), buf.nbytes, peer, _sptr(stream))

    def barrier(self, stream=None) -> None:
        _lib.call("fmi_comm_barrier", self.handle, _sptr(stream))
