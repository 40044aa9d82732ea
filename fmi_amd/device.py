"""Host-side handle to the gfx950 bucket-reduction engine (thin layer over include/fmi_dev.h).

Names follow FMI's vocabulary: a *bucket* is one peer's contiguous buffer (reference
include/comm/Data.h:50-73, `Data<std::vector<A>>`), an *op* is one of the reference's built-in
reduction functions (reference python/PythonCommunicator.h:131-149), and the P-way entry points
reproduce the combine order of a reference collective (reference src/comm/PeerToPeer.cpp).
"""
from __future__ import annotations

import ctypes
import enum
from typing import Optional, Sequence

import numpy as np

from . import _lib


class Op(enum.IntEnum):
    """Reference Python op enum SUM/PROD/MAX/MIN (reference python/PythonCommunicator.h:13-15), and AVG, the mean
    over the peers (fmi_dev.h's FMI_OP_AVG; 4 is the reference's CUSTOM and stays unassigned): the SUM program's
    value times the rounded reciprocal of the peer count, float dtypes, in the calls that produce a reduction result
    (reduce_tree, comm.allreduce / reduce / allreduce_host)."""
    SUM = 0
    PROD = 1
    MAX = 2
    MIN = 3
    AVG = 5


class DType(enum.IntEnum):
    """fmi_dtype_t. F32 / F64 / I32 / I64 run every kernel, and so do F16 (IEEE binary16) and BF16 (the upper half
    of binary32): the pairwise kernels and every fused / one-pass P-way form, at all five algorithms and any number
    of peers; every combine widens to f32 and rounds back to the storage type (include/fmi_dev.h). The other integer
    widths run the pairwise kernel, and their P-way programs run as pairwise passes (as unaligned buckets do).
    F8E4M3 / F8E5M2 are the two OCP 8-bit floats (e4m3fn, e5m2; non-saturating narrowing): the pairwise kernels, fused
    P-way kernels with accumulate_f32 up to 16 peers, and pairwise passes for the plain P-way programs."""
    F32 = 0
    F64 = 1
    I32 = 2
    I64 = 3
    U32 = 4
    U64 = 5
    I8 = 6
    U8 = 7
    I16 = 8
    U16 = 9
    F16 = 10
    BF16 = 11
    F8E4M3 = 12
    F8E5M2 = 13
    # The scale bytes of an MX bucket (E8M0: 2^(e - 127), 255 = NaN), one per 32 elements, over np.uint8. A label of this
    # binding alone (include/fmi_dev.h reserves the value): no C-ABI call takes it as an element dtype.
    F8E8M0 = 14
    # The OCP 4-bit float E2M1, the element of an MXFP4 bucket: two elements to a byte over np.uint8 (element 2k in bits
    # 3:0 of byte k, element 2k + 1 in bits 7:4), so a Bucket of n ELEMENTS holds (n + 1) // 2 bytes. Valid in the MX
    # calls alone (reduce_tree_mx, mx_quantize, mx_dequantize, Comm.allreduce_mx): every other call raises ValueError.
    F4E2M1 = 15
    # The two OCP 6-bit floats, the elements of an MXFP6 bucket: four elements to three bytes over np.uint8 (element i in
    # bits 6 i .. 6 i + 5 of the little-endian bit string), so a Bucket of n ELEMENTS holds (3 n + 3) // 4 bytes. Valid
    # in the MX calls alone, like F4E2M1.
    F6E2M3 = 16
    F6E3M2 = 17


FP6_DTYPES = (DType.F6E2M3, DType.F6E3M2)
# what an MX bucket's elements can be
MX_DTYPES = (DType.F8E4M3, DType.F8E5M2, DType.F4E2M1) + FP6_DTYPES


# fmi_dev.h's FMI_ACC_F32: ORed into the dtype argument of a P-way call on F16 / BF16 / F8E4M3 / F8E5M2 buckets, the program's values
# are kept in f32 and every stored output is rounded to the storage type once (`accumulate_f32=True` below).
ACC_F32 = 0x100


def acc_dtype(dtype: "DType", accumulate_f32: bool) -> int:
    """The dtype argument of a P-way call: the storage dtype, with ACC_F32 when `accumulate_f32`."""
    if not accumulate_f32:
        return int(dtype)
    if dtype not in (DType.F16, DType.BF16, DType.F8E4M3, DType.F8E5M2):
        raise ValueError(f"accumulate_f32 needs F16 or BF16 (or F8E4M3 / F8E5M2) buckets, got {DType(dtype).name}")
    return int(dtype) | ACC_F32


class Alg(enum.IntEnum):
    """Evaluation orders of the reference collectives (src/comm/PeerToPeer.cpp)."""
    ALLREDUCE = 0   # allreduce_no_order  :96-130
    REDUCE = 1      # reduce_no_order     :59-84
    REDUCE_LTR = 2  # reduce_ltr          :44-57
    SCAN = 3        # scan_no_order       :154-184
    SCAN_LTR = 4    # scan_ltr            :141-152


class Tune(enum.IntEnum):
    PAIR_VARIANT = 0
    PAIR_UNROLL = 1
    BLOCK = 2
    GRID_PER_CU = 3
    HOST_CHUNK = 4
    HOST_ZERO_COPY = 5
    FUSED_INFLIGHT_KIB = 6
    BLOCKS_ONE_PASS = 7
    COMM_A2A = 8
    COMM_GATHER = 9
    COMM_PIPELINE = 10
    FUSED_POLICY = 11
    PAIR_SC1_OF_8 = 12
    COMM_ONE_RANK_EXCHANGE = 13
    ALLOC_SLOTS = 14
    COMM_SHARD_SKEW = 15


NP_DTYPE = {DType.F32: np.float32, DType.F64: np.float64, DType.I32: np.int32, DType.I64: np.int64,
            DType.U32: np.uint32, DType.U64: np.uint64, DType.I8: np.int8, DType.U8: np.uint8, DType.I16: np.int16,
            DType.U16: np.uint16, DType.F16: np.float16}
# numpy has no bfloat16 and no 8-bit floats: a BF16 bucket moves its elements' raw bits as np.uint16, an F8E4M3 /
# F8E5M2 bucket as np.uint8 (np.uint8 alone keeps meaning U8)
_HOST_DTYPE = {**NP_DTYPE, DType.BF16: np.uint16, DType.F8E4M3: np.uint8, DType.F8E5M2: np.uint8, DType.F8E8M0: np.uint8,
               DType.F4E2M1: np.uint8, DType.F6E2M3: np.uint8, DType.F6E3M2: np.uint8}


def storage_bytes(dtype: "DType", n: int) -> int:
    """The bytes a bucket of n elements takes: n times the element size, (n + 1) // 2 for the packed F4E2M1, or
    (3 n + 3) // 4 for the packed F6E2M3 / F6E3M2."""
    if dtype == DType.F4E2M1:
        return (int(n) + 1) // 2
    if dtype in FP6_DTYPES:
        return (3 * int(n) + 3) // 4
    return int(n) * np.dtype(_HOST_DTYPE[dtype]).itemsize


def refuse_fp4(who: str, *buckets) -> None:
    """F4E2M1, F6E2M3 and F6E3M2 buckets are valid in the MX calls alone: every other call refuses them before it
    reaches the library."""
    for b in buckets:
        dt = getattr(b, "dtype", None)
        if dt == DType.F4E2M1 or dt in FP6_DTYPES:
            raise ValueError(f"{who}: {DType(dt).name} buckets are valid only in reduce_tree_mx, mx_quantize, mx_dequantize and "
                             f"Comm.allreduce_mx")


def fp4_pack(nibbles) -> np.ndarray:
    """E2M1 codes (one per element, 0..15) packed two to a byte: element 2k in bits 3:0 of byte k, element 2k + 1 in bits
    7:4; an odd count leaves the last byte's high nibble 0."""
    c = np.ascontiguousarray(nibbles, dtype=np.uint8).ravel()
    if c.size and int(c.max()) > 15:
        raise ValueError("fp4_pack: codes must be in 0..15")
    if c.size % 2:
        c = np.concatenate([c, np.zeros(1, np.uint8)])
    return (c[0::2] | (c[1::2] << 4)).astype(np.uint8)


def fp4_unpack(packed, n: int) -> np.ndarray:
    """The n E2M1 codes of a packed bucket ((n + 1) // 2 bytes): the inverse of fp4_pack."""
    b = np.ascontiguousarray(packed, dtype=np.uint8).ravel()
    if b.size != (int(n) + 1) // 2:
        raise ValueError(f"fp4_unpack: {n} elements are {(int(n) + 1) // 2} bytes, got {b.size}")
    out = np.empty(2 * b.size, np.uint8)
    out[0::2] = b & 0xF
    out[1::2] = b >> 4
    return out[:int(n)]


def fp6_pack(codes) -> np.ndarray:
    """FP6 codes (one per element, 0..63) packed four to three bytes: element i in bits 6 i .. 6 i + 5 of the
    little-endian bit string; the unused high bits of the last byte are 0."""
    c = np.ascontiguousarray(codes, dtype=np.uint8).ravel()
    if c.size and int(c.max()) > 63:
        raise ValueError("fp6_pack: codes must be in 0..63")
    n = c.size
    q = np.zeros((n + 3) // 4 * 4, np.uint32)
    q[:n] = c
    q = q.reshape(-1, 4)
    w = q[:, 0] | (q[:, 1] << 6) | (q[:, 2] << 12) | (q[:, 3] << 18)
    out = np.stack([w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF], axis=1).astype(np.uint8).ravel()
    return out[:(3 * n + 3) // 4].copy()


def fp6_unpack(packed, n: int) -> np.ndarray:
    """The n FP6 codes of a packed bucket ((3 n + 3) // 4 bytes): the inverse of fp6_pack."""
    b = np.ascontiguousarray(packed, dtype=np.uint8).ravel()
    n = int(n)
    if b.size != (3 * n + 3) // 4:
        raise ValueError(f"fp6_unpack: {n} elements are {(3 * n + 3) // 4} bytes, got {b.size}")
    t = np.zeros((n + 3) // 4 * 3, np.uint32)
    t[:b.size] = b
    t = t.reshape(-1, 3)
    w = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
    out = np.stack([w & 63, (w >> 6) & 63, (w >> 12) & 63, (w >> 18) & 63], axis=1).astype(np.uint8).ravel()
    return out[:n].copy()


def dtype_of(arr_or_dtype) -> DType:
    if isinstance(arr_or_dtype, np.ndarray):
        dt = arr_or_dtype.dtype
    else:
        dt = np.dtype(arr_or_dtype)
    for k, v in NP_DTYPE.items():
        if np.dtype(v) == dt:
            return k
    raise TypeError(f"unsupported bucket dtype {dt}; FMI device buckets are f16, f32, f64 or "
                    f"8/16/32/64-bit integers (bf16: pass DType.BF16 and move np.uint16 bit patterns)")


def itemsize_of(dtype) -> int:
    """Bytes per element of a numpy dtype or a DType."""
    dt = dtype if isinstance(dtype, DType) else dtype_of(dtype)
    return np.dtype(_HOST_DTYPE[dt]).itemsize


def _ptr(x) -> Optional[int]:
    if x is None:
        return None
    if isinstance(x, Bucket):
        return x.ptr
    if isinstance(x, int):
        return x
    raise TypeError(f"expected a Bucket or a raw device pointer, got {type(x)}")


def _sptr(stream) -> Optional[int]:
    if stream is None:
        return None
    return stream.handle if isinstance(stream, Stream) else int(stream)


# ----------------------------------------------------------------------------------------------------
# device / memory
# ----------------------------------------------------------------------------------------------------
def device_count() -> int:
    c = ctypes.c_int(0)
    _lib.call("fmi_dev_count", ctypes.byref(c))
    return c.value


def init(device: int = 0) -> None:
    _lib.call("fmi_dev_init", device)


def finalize() -> None:
    _lib.call("fmi_dev_finalize")


def sync() -> None:
    _lib.call("fmi_dev_sync")


def describe() -> str:
    buf = ctypes.create_string_buffer(512)
    _lib.call("fmi_dev_describe", buf, len(buf))
    return buf.value.decode()


def pci_bus_id(device: int) -> str:
    """PCI bus id of a visible device ("dddd:bb:dd.f")."""
    buf = ctypes.create_string_buffer(64)
    _lib.call("fmi_dev_pci_bus_id", int(device), buf, len(buf))
    return buf.value.decode()


class Bucket:
    """A device-resident bucket of `n` elements of `dtype` (owns its HBM allocation unless `view`).

    `dtype` is a numpy dtype or a DType. numpy has no bfloat16, so a bf16 bucket is created with the explicit
    DType.BF16 and uploads / downloads np.uint16 bit patterns (np.uint16 itself keeps meaning DType.U16)."""

    def __init__(self, n: int, dtype, ptr: Optional[int] = None, owner: Optional["Bucket"] = None):
        self.dtype = dtype_of(dtype) if not isinstance(dtype, DType) else dtype
        self.n = int(n)
        self.itemsize = np.dtype(_HOST_DTYPE[self.dtype]).itemsize
        self._owner = owner
        if ptr is None:
            p = ctypes.c_void_p()
            _lib.call("fmi_dev_alloc", ctypes.byref(p), self.nbytes)
            self.ptr = p.value
            self._owns = True
        else:
            self.ptr = ptr
            self._owns = False

    @property
    def nbytes(self) -> int:
        return storage_bytes(self.dtype, self.n)

    @classmethod
    def group(cls, count: int, n: int, dtype) -> list:
        """`count` buckets that one kernel streams together (a fused kernel's peers and outputs, a pair's two
        operands): fmi_dev_alloc_group puts bucket j in 4 KiB slot j mod 16, whatever was allocated before
        (DESIGN §4)."""
        dt = dtype_of(dtype) if not isinstance(dtype, DType) else dtype
        nbytes = storage_bytes(dt, n)
        ptrs = (ctypes.c_void_p * max(int(count), 1))()
        _lib.call("fmi_dev_alloc_group", ptrs, int(count), nbytes)
        out = []
        for j in range(int(count)):
            b = cls(n, dt, ptr=ptrs[j])
            b._owns = True
            out.append(b)
        return out

    @classmethod
    def from_numpy(cls, arr: np.ndarray, stream=None) -> "Bucket":
        arr = np.ascontiguousarray(arr)
        b = cls(arr.size, dtype_of(arr))
        b.upload(arr, stream)
        return b

    def view(self, offset: int, n: int) -> "Bucket":
        """Sub-bucket starting `offset` elements in (used to exercise unaligned buckets). An F4E2M1 bucket needs an even
        element offset, an F6E2M3 / F6E3M2 bucket a multiple of 4: a view starts on a byte."""
        if offset < 0 or offset + n > self.n:
            raise ValueError("view out of range")
        if self.dtype == DType.F4E2M1:
            if offset % 2:
                raise ValueError("view: an F4E2M1 bucket needs an even element offset (two elements to a byte)")
            return Bucket(n, self.dtype, ptr=self.ptr + offset // 2, owner=self)
        if self.dtype in FP6_DTYPES:
            if offset % 4:
                raise ValueError(f"view: an {self.dtype.name} bucket needs an element offset that is a multiple of 4 (four elements "
                                 f"to three bytes)")
            return Bucket(n, self.dtype, ptr=self.ptr + offset // 4 * 3, owner=self)
        return Bucket(n, self.dtype, ptr=self.ptr + offset * self.itemsize, owner=self)

    def upload(self, arr: np.ndarray, stream=None) -> None:
        arr = np.ascontiguousarray(arr, dtype=_HOST_DTYPE[self.dtype])
        if arr.nbytes != self.nbytes:  # F4E2M1: the packed bytes, (n + 1) // 2 of them
            raise ValueError(f"size mismatch: bucket has {self.n} elements, array {arr.size}")
        _lib.call("fmi_dev_h2d_async", self.ptr, arr.ctypes.data, self.nbytes, _sptr(stream))
        _lib.call("fmi_stream_sync", _sptr(stream))

    def numpy(self, stream=None) -> np.ndarray:
        out = np.empty(self.nbytes // self.itemsize, dtype=_HOST_DTYPE[self.dtype])  # F4E2M1: the packed bytes
        _lib.call("fmi_dev_d2h_async", out.ctypes.data, self.ptr, self.nbytes, _sptr(stream))
        _lib.call("fmi_stream_sync", _sptr(stream))
        return out

    def fill_synthetic(self, seed: int, peer: int, stream=None, first: int = 0) -> "Bucket":
        """Elements [first, first + n) of peer `peer`'s synthetic bucket (SURVEY.md §8d generator)."""
        refuse_fp4("fill_synthetic", self)
        _lib.call("fmi_dev_fill_synthetic_at", int(self.dtype), self.ptr, self.n, seed, peer, int(first),
                  _sptr(stream))
        return self

    def copy_from(self, other: "Bucket", stream=None) -> None:
        if other.nbytes != self.nbytes:
            raise ValueError("size mismatch")
        _lib.call("fmi_dev_d2d_async", self.ptr, other.ptr, self.nbytes, _sptr(stream))

    def free(self) -> None:
        if self._owns and self.ptr:
            _lib.call("fmi_dev_free", self.ptr)
        self.ptr = 0
        self._owns = False

    def __del__(self):
        try:
            if getattr(self, "_owns", False) and self.ptr:
                _lib.load().fmi_dev_free(self.ptr)
        except Exception:
            pass


class Stream:
    def __init__(self):
        h = ctypes.c_void_p()
        _lib.call("fmi_stream_create", ctypes.byref(h))
        self.handle = h.value

    def sync(self) -> None:
        _lib.call("fmi_stream_sync", self.handle)

    def destroy(self) -> None:
        if self.handle:
            _lib.call("fmi_stream_destroy", self.handle)
            self.handle = None


class Graph:
    """A launch sequence recorded once and replayed as one submission (fmi_graph_*): many small bucket
    combines, where launch cost rather than HBM is the limit.

        g = Graph.capture(stream, lambda: [reduce_pair(Op.SUM, a, b, stream=stream) for a, b in pairs])
        g.launch(stream)   # every combine again, same buckets
    """

    def __init__(self, handle: int):
        self.handle = handle

    @classmethod
    def capture(cls, stream: "Stream", record) -> "Graph":
        _lib.call("fmi_graph_capture_begin", stream.handle)
        h = ctypes.c_void_p()
        try:
            record()
        finally:  # always end the capture, so a failure inside `record` leaves the stream usable
            end_rc = _lib.load().fmi_graph_capture_end(stream.handle, ctypes.byref(h))
        if end_rc != 0:
            raise _lib.FmiError(end_rc, _lib.last_error())
        return cls(h.value)

    def launch(self, stream=None) -> None:
        _lib.call("fmi_graph_launch", self.handle, _sptr(stream))

    def destroy(self) -> None:
        if self.handle:
            _lib.call("fmi_graph_destroy", self.handle)
            self.handle = None


class Event:
    def __init__(self):
        h = ctypes.c_void_p()
        _lib.call("fmi_event_create", ctypes.byref(h))
        self.handle = h.value

    def record(self, stream=None) -> "Event":
        _lib.call("fmi_event_record", self.handle, _sptr(stream))
        return self

    def sync(self) -> None:
        _lib.call("fmi_event_sync", self.handle)

    def wait_on(self, stream=None) -> None:
        """Make later work on `stream` (None = library stream) wait for this event."""
        _lib.call("fmi_stream_wait_event", _sptr(stream), self.handle)

    def elapsed_ms(self, end: "Event") -> float:
        ms = ctypes.c_float()
        _lib.call("fmi_event_elapsed_ms", ctypes.byref(ms), self.handle, end.handle)
        return float(ms.value)

    def destroy(self) -> None:
        if self.handle:
            _lib.call("fmi_event_destroy", self.handle)
            self.handle = None


# ----------------------------------------------------------------------------------------------------
# hot path
# ----------------------------------------------------------------------------------------------------
def reduce_pair(op: Op, inout: Bucket, src: Bucket, n: Optional[int] = None, stream=None) -> None:
    """inout = op(inout, src) elementwise — one reference `f.f(a, b)` (include/Communicator.h:180-189)."""
    n = inout.n if n is None else n
    refuse_fp4("reduce_pair", inout, src)
    if src.dtype != inout.dtype or src.n < n or inout.n < n:
        raise ValueError("reduce_pair: buckets must share dtype and hold n elements")
    _lib.call("fmi_dev_reduce_pair", int(op), int(inout.dtype), inout.ptr, src.ptr, n, _sptr(stream))


class _PairDesc(ctypes.Structure):
    _fields_ = [("inout", ctypes.c_void_p), ("in_", ctypes.c_void_p), ("n", ctypes.c_size_t)]


def reduce_pair_batch(op: Op, pairs: Sequence, stream=None) -> None:
    """inout = op(inout, in) for every (inout, in) bucket pair, batched into as few launches as possible
    (fmi_dev_reduce_pair_batch): for many small buckets. All buckets share one dtype."""
    if not pairs:
        return
    dtype = pairs[0][0].dtype
    for a, b in pairs:
        refuse_fp4("reduce_pair_batch", a, b)
        if a.dtype != dtype or b.dtype != dtype or b.n < a.n:
            raise ValueError("reduce_pair_batch: one dtype for every bucket, and each `in` at least as long as its inout")
    descs = (_PairDesc * len(pairs))(*[_PairDesc(a.ptr, b.ptr, a.n) for a, b in pairs])
    _lib.call("fmi_dev_reduce_pair_batch", int(op), int(dtype), ctypes.cast(descs, ctypes.c_void_p), len(pairs),
              _sptr(stream))


def combine(op: Op, out: Bucket, a: Bucket, b: Bucket, stream=None) -> None:
    refuse_fp4("combine", out, a, b)
    if not (out.dtype == a.dtype == b.dtype) or not (out.n == a.n == b.n):
        raise ValueError("combine: buckets must share dtype and length")
    _lib.call("fmi_dev_combine", int(op), int(out.dtype), out.ptr, a.ptr, b.ptr, out.n, _sptr(stream))


def _ptr_array(buckets: Sequence[Bucket]):
    arr = (ctypes.c_void_p * len(buckets))()
    for i, b in enumerate(buckets):
        arr[i] = b.ptr
    return arr


def reduce_tree(op: Op, alg: Alg, out: Bucket, ins: Sequence[Bucket], rank: int = 0, stream=None,
                accumulate_f32: bool = False) -> None:
    """P-way reduction with a reference collective's bracketing (see include/fmi_dev.h). accumulate_f32 (F16 / BF16 /
    F8E4M3 / F8E5M2 buckets): the same program on f32 values, the result rounded to the storage type once."""
    refuse_fp4("reduce_tree", out, *ins)
    dtype = acc_dtype(out.dtype, accumulate_f32)
    _check_peers(out, ins)
    _lib.call("fmi_dev_reduce_tree", int(op), dtype, int(alg), out.ptr, _ptr_array(ins), len(ins), rank,
              out.n, _sptr(stream))


def _f32_word(b, what: str, n: int = 1) -> Optional[int]:
    if b is None:
        return None
    if not isinstance(b, Bucket) or b.dtype != DType.F32 or b.n < n:
        raise ValueError(f"{what} must be an F32 bucket of at least {n} element(s)")
    return b.ptr


def reduce_tree_scaled(alg: Alg, out: Bucket, ins: Sequence[Bucket], in_scales: Bucket, out_scale: Optional[Bucket] = None,
                       amax: Optional[Bucket] = None, rank: int = 0, stream=None) -> None:
    """The scaled sum of F8E4M3 / F8E5M2 buckets (fmi_dev_reduce_tree_scaled): every input times its own scale in f32,
    the f32 SUM program of `alg`, amax of the sum folded into `amax`, the sum times `out_scale`, stored once into `out`:
    a bucket of the inputs' dtype (non-saturating narrowing) or an F32 bucket. in_scales (one per peer), out_scale and
    amax are F32 buckets: the scales live on the device, so a captured graph replays with new ones. One fused kernel at
    2..16 peers on 16-B aligned buckets."""
    if not ins:
        raise ValueError("need at least one peer bucket")
    dtype = ins[0].dtype
    if dtype not in (DType.F8E4M3, DType.F8E5M2):
        raise ValueError(f"reduce_tree_scaled needs F8E4M3 or F8E5M2 input buckets, got {DType(dtype).name}")
    _check_peers(ins[0], ins)
    if out.n != ins[0].n or out.dtype not in (dtype, DType.F32):
        raise ValueError("reduce_tree_scaled: `out` must hold the inputs' length in their dtype or in F32")
    _lib.call("fmi_dev_reduce_tree_scaled", int(Op.SUM), int(dtype), int(alg), int(out.dtype), out.ptr, _ptr_array(ins),
              _f32_word(in_scales, "in_scales", len(ins)), _f32_word(out_scale, "out_scale"), _f32_word(amax, "amax"),
              len(ins), rank, out.n, _sptr(stream))


MX_BLOCK = 32  # elements per scale byte of an MX bucket


def mx_blocks(n: int) -> int:
    """The number of scale bytes of an MX bucket of n elements: ceil(n / 32)."""
    return (int(n) + MX_BLOCK - 1) // MX_BLOCK


def _mx_scales(b, what: str, n: int) -> int:
    if not isinstance(b, Bucket) or b.dtype not in (DType.F8E8M0, DType.U8):
        raise ValueError(f"{what} must be an F8E8M0 (or U8) bucket of scale bytes")
    if b.n != mx_blocks(n):
        raise ValueError(f"{what} must hold ceil(n / 32) = {mx_blocks(n)} scale bytes for {n} elements, got {b.n}")
    return b.ptr


def _mx_elements(who: str, what: str, b: Bucket) -> DType:
    if b.dtype not in MX_DTYPES:
        raise ValueError(f"{who} needs F8E4M3 or F8E5M2 {what}, got {DType(b.dtype).name}; F4E2M1 (MXFP4) is the third "
                         f"element type an MX bucket can have, F6E2M3 and F6E3M2 (MXFP6) the fourth and fifth")
    return b.dtype


def _sr_seed(who: str, seed, out: Bucket, first: int) -> int:
    """The device word of a stochastic-rounding call: a U64 bucket of one element."""
    if not isinstance(seed, Bucket) or seed.dtype != DType.U64 or seed.n != 1:
        raise ValueError(f"{who}: `seed` must be a U64 bucket of one element (the Philox key, in device memory)")
    if out.dtype == DType.F32:
        raise ValueError(f"{who}: stochastic rounding needs an output of the element type: an F32 output has nothing to round")
    if not 0 <= int(first) < 1 << 64:
        raise ValueError(f"{who}: `first` must be an unsigned 64-bit stream position")
    return seed.ptr


def reduce_tree_mx(op: Op, alg: Alg, out: Bucket, out_scales: Optional[Bucket], ins: Sequence[Bucket],
                   in_scales: Sequence[Bucket], rank: int = 0, stream=None, seed: Optional[Bucket] = None,
                   first: int = 0) -> None:
    """The sum (Op.SUM) or mean (Op.AVG) of block-scaled (MX) F8E4M3 / F8E5M2 (MXFP8), F4E2M1 (MXFP4, packed two
    elements to a byte; the scale rule at EMAX = 2) or F6E2M3 / F6E3M2 (MXFP6, packed four elements to three bytes; the
    largest elements 7.5 and 28) buckets (fmi_dev_reduce_tree_mx): every
    input element times its block's E8M0 scale in f32, the f32 SUM program of `alg`, then either stored as F32 (`out` an
    F32 bucket, out_scales None) or requantized: per block of 32 the smallest power-of-two scale that brings the block's
    largest magnitude within the element type, into `out_scales`, and the scaled sum narrowed into `out`. in_scales[p]
    and out_scales are F8E8M0 buckets of ceil(n / 32) bytes. One fused kernel at 2..16 peers on 16-B aligned element
    buckets; bit-exact and deterministic.
    seed: a U64 bucket of one element selects stochastic rounding (fmi_dev_reduce_tree_mx_sr): the same scale bytes, every
    element rounded to one of its two grid neighbours by 16 Philox bits keyed by (the word in `seed`, first + its index).
    `first`, a multiple of 32, is the stream position of element 0: a bucket reduced in pieces passes each piece's offset."""
    if not ins:
        raise ValueError("need at least one peer bucket")
    dtype = _mx_elements("reduce_tree_mx", "input buckets", ins[0])
    _check_peers(ins[0], ins)
    if out.n != ins[0].n or out.dtype not in (dtype, DType.F32):
        raise ValueError("reduce_tree_mx: `out` must hold the inputs' length in their dtype or in F32")
    if len(in_scales) != len(ins):
        raise ValueError("reduce_tree_mx: one in_scales bucket per input")
    if out.dtype != DType.F32 and out_scales is None:
        raise ValueError("reduce_tree_mx: out_scales is missing: only an F32 output has no scale bytes")
    sptrs = (ctypes.c_void_p * len(ins))(*[_mx_scales(b, f"in_scales[{p}]", out.n) for p, b in enumerate(in_scales)])
    if seed is not None:
        word = _sr_seed("reduce_tree_mx", seed, out, first)
        _lib.call("fmi_dev_reduce_tree_mx_sr", int(op), int(dtype), int(alg), out.ptr, _mx_scales(out_scales, "out_scales", out.n),
                  _ptr_array(ins), sptrs, word, int(first), len(ins), rank, out.n, _sptr(stream))
        return
    _lib.call("fmi_dev_reduce_tree_mx", int(op), int(dtype), int(alg), int(out.dtype), out.ptr,
              None if out_scales is None else _mx_scales(out_scales, "out_scales", out.n), _ptr_array(ins), sptrs,
              len(ins), rank, out.n, _sptr(stream))


def mx_quantize(out: Bucket, out_scales: Bucket, src: Bucket, stream=None, seed: Optional[Bucket] = None, first: int = 0) -> None:
    """An F32 / F16 / BF16 bucket into an MX bucket (fmi_dev_mx_quantize): per block of 32 elements the scale byte of
    reduce_tree_mx, into `out_scales`, and the elements narrowed under it into `out` (F8E4M3 / F8E5M2). seed, first: as
    reduce_tree_mx's (fmi_dev_mx_quantize_sr)."""
    dtype = _mx_elements("mx_quantize", "output bucket", out)
    if src.dtype not in (DType.F32, DType.F16, DType.BF16) or src.n != out.n:
        raise ValueError("mx_quantize: `src` must be an F32, F16 or BF16 bucket of out's length")
    if seed is not None:
        _lib.call("fmi_dev_mx_quantize_sr", int(dtype), out.ptr, _mx_scales(out_scales, "out_scales", out.n), int(src.dtype),
                  src.ptr, out.n, _sr_seed("mx_quantize", seed, out, first), int(first), _sptr(stream))
        return
    _lib.call("fmi_dev_mx_quantize", int(dtype), out.ptr, _mx_scales(out_scales, "out_scales", out.n), int(src.dtype),
              src.ptr, out.n, _sptr(stream))


def mx_quantize_sr_host(dtype, src, seed: int, first: int = 0):
    """fmi_dev_mx_quantize_sr of a float32 numpy array on the host (fmi_host_mx_quantize_sr): (element bytes, scale bytes)
    as np.uint8 arrays, the bytes the device call stores for the same (seed, first). dtype: F8E4M3, F8E5M2, F4E2M1
    (packed, ceil(n / 2) bytes) or F6E2M3 / F6E3M2 (packed, ceil(3 n / 4) bytes). Needs no device."""
    dtype = DType(dtype)
    if dtype not in MX_DTYPES:
        raise ValueError(f"mx_quantize_sr_host needs F8E4M3, F8E5M2 or F4E2M1, got {dtype.name}")
    a = np.ascontiguousarray(src, np.float32).ravel()
    n = a.size
    out = np.zeros(storage_bytes(dtype, n), np.uint8)
    scales = np.zeros(mx_blocks(n), np.uint8)
    if not 0 <= int(seed) < 1 << 64 or not 0 <= int(first) < 1 << 64:
        raise ValueError("mx_quantize_sr_host: seed and first are unsigned 64-bit values")
    _lib.call("fmi_host_mx_quantize_sr", int(dtype), out.ctypes.data, scales.ctypes.data,
              a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), n, int(seed), int(first))
    return out, scales


def mx_dequantize(dst: Bucket, src: Bucket, src_scales: Bucket, stream=None) -> None:
    """An MX bucket into an F32 / F16 / BF16 bucket (fmi_dev_mx_dequantize): dst = narrow_dst(widen(src) * scale)."""
    dtype = _mx_elements("mx_dequantize", "source bucket", src)
    if dst.dtype not in (DType.F32, DType.F16, DType.BF16) or dst.n != src.n:
        raise ValueError("mx_dequantize: `dst` must be an F32, F16 or BF16 bucket of src's length")
    _lib.call("fmi_dev_mx_dequantize", int(dst.dtype), dst.ptr, int(dtype), src.ptr, _mx_scales(src_scales, "src_scales", src.n),
              src.n, _sptr(stream))


def mean_scale(inout: Bucket, P: int, n: Optional[int] = None, stream=None) -> None:
    """inout = inout * fl(1 / P) in place (fmi_dev_mean_scale): Op.AVG's last step alone, for a SUM that went through
    an exchange of the caller's own. Float buckets; f16 / bf16 multiply in f32 and round to storage once."""
    n = inout.n if n is None else n
    refuse_fp4("mean_scale", inout)
    if inout.n < n:
        raise ValueError("mean_scale: the bucket must hold n elements")
    _lib.call("fmi_dev_mean_scale", int(inout.dtype), inout.ptr, n, int(P), _sptr(stream))


def convert(dst: Bucket, src: Bucket, n: Optional[int] = None, stream=None) -> None:
    """dst = src converted to dst's dtype (fmi_dev_convert), between F32, F16, BF16, F8E4M3 and F8E5M2: the value goes
    through f32, one rounding in all (to the 8-bit floats non-saturating). How f32 / bf16 data gets into an 8-bit float
    bucket. dst may be src at equal element size."""
    n = dst.n if n is None else n
    refuse_fp4("convert", dst, src)
    if dst.n < n or src.n < n:
        raise ValueError("convert: both buckets must hold n elements")
    _lib.call("fmi_dev_convert", int(dst.dtype), dst.ptr, int(src.dtype), src.ptr, n, _sptr(stream))


def scan_peers(op: Op, alg: Alg, outs: Sequence[Bucket], ins: Sequence[Bucket], stream=None,
               accumulate_f32: bool = False) -> None:
    """Peer-axis inclusive scan with the bracketing of reference scan_no_order / scan_ltr. accumulate_f32 (F16 /
    BF16 / F8E4M3 / F8E5M2 buckets): the same program on f32 values, every prefix rounded to the storage type once."""
    if len(outs) != len(ins):
        raise ValueError("scan_peers: one output bucket per peer")
    refuse_fp4("scan_peers", *outs, *ins)
    dtype = acc_dtype(outs[0].dtype, accumulate_f32)
    _check_peers(outs[0], ins)  # O(P): every bucket, in or out, against the first output
    _check_peers(outs[0], outs)
    _lib.call("fmi_dev_scan_peers", int(op), dtype, int(alg), _ptr_array(outs), _ptr_array(ins),
              len(ins), outs[0].n, _sptr(stream))


def host_reduce_pair(op: Op, inout: np.ndarray, src: np.ndarray, dtype: Optional[DType] = None) -> None:
    """inout = op(inout, src) for host arrays, streamed through the device (H2D, kernel, D2H). `dtype`: the element
    type where the arrays carry raw bits (DType.BF16 over np.uint16, DType.F8E4M3 / F8E5M2 over np.uint8); None = the
    arrays' own."""
    if inout.dtype != src.dtype or inout.size != src.size:
        raise ValueError("host_reduce_pair: arrays must share dtype and size")
    if not (inout.flags.c_contiguous and src.flags.c_contiguous):
        raise ValueError("host_reduce_pair: arrays must be contiguous")
    dt = dtype_of(inout) if dtype is None else DType(dtype)
    if dt == DType.F4E2M1 or dt in FP6_DTYPES:
        raise ValueError(f"host_reduce_pair: {dt.name} is valid only in the MX calls")
    if np.dtype(_HOST_DTYPE[dt]).itemsize != inout.dtype.itemsize:
        raise ValueError("host_reduce_pair: the arrays' element size is not the dtype's")
    _lib.call("fmi_host_reduce_pair", int(op), int(dt), inout.ctypes.data, src.ctypes.data, inout.size)


class PinnedArray:
    """A numpy array over page-locked host memory (fmi_host_pin_alloc) — the recv-buffer kind the
    zero-copy host path combines in place over PCIe. Free with .free() (or on garbage collection)."""

    def __init__(self, n: int, dtype):
        self.dtype = np.dtype(dtype)
        nbytes = max(1, int(n) * self.dtype.itemsize)
        p = ctypes.c_void_p()
        _lib.call("fmi_host_pin_alloc", ctypes.byref(p), nbytes)
        self.ptr = p.value
        raw = (ctypes.c_char * nbytes).from_address(self.ptr)
        self.array = np.frombuffer(raw, dtype=self.dtype, count=int(n))

    def free(self) -> None:
        if self.ptr:
            self.array = None
            _lib.call("fmi_host_pin_free", self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                _lib.load().fmi_host_pin_free(self.ptr)
        except Exception:
            pass


class HostRegistration:
    """Page-lock an existing contiguous numpy array in place (fmi_host_register), so fmi_host_reduce_pair
    combines it zero-copy and the host pipelines move it at DMA rate. For recv buffers reused across many
    collectives: registering costs about one copy of the array. The array must outlive the registration.
    Use as a context manager, or call .close()."""

    def __init__(self, arr: np.ndarray):
        if not arr.flags.c_contiguous or arr.nbytes == 0:
            raise ValueError("HostRegistration: needs a non-empty contiguous array")
        self.array = arr
        self.ptr = arr.ctypes.data
        _lib.call("fmi_host_register", self.ptr, arr.nbytes)

    def close(self) -> None:
        if self.ptr:
            _lib.call("fmi_host_unregister", self.ptr)
            self.ptr = None
            self.array = None

    def __enter__(self) -> "HostRegistration":
        return self

    def __exit__(self, *exc) -> None:
        self.close()


def _check_peers(out: Bucket, ins: Sequence[Bucket]) -> None:
    if not ins:
        raise ValueError("need at least one peer bucket")
    for b in ins:
        if b.dtype != out.dtype or b.n != out.n:
            raise ValueError("all peer buckets must share dtype and length")


def schedule_expr(alg: Alg, P: int, rank: int) -> str:
    size = 1 << 16
    while True:
        buf = ctypes.create_string_buffer(size)
        status = _lib.load().fmi_schedule_expr(int(alg), P, rank, buf, len(buf))
        msg = _lib.last_error() if status else ""
        if status and "buffer too small" in msg:  # "(<bytes> needed)"
            size = int(msg.split("(")[1].split()[0])
            continue
        _lib.check(status)
        return buf.value.decode()


def tune_set(key: Tune, value: int) -> None:
    _lib.call("fmi_tune_set", int(key), int(value))


def tune_get(key: Tune) -> int:
    v = ctypes.c_longlong()
    _lib.call("fmi_tune_get", int(key), ctypes.byref(v))
    return v.value
