"""Guarded, poisoned device buckets: the one harness of the containment tests ("Containment").

An entry point must write exactly the bytes of its outputs and no byte of an input it does not own. Comparing the n
output elements alone cannot show either: an element the kernel never wrote can hold the right bits from an earlier
launch at the same address, and a store past the end lands in somebody else's allocation. So:

    Guarded(n, dtype, offset)   one allocation: [ front guard 4 KiB | offset elements of slack | body | back guard 8 KiB ]
                                guards and slack hold GUARD_BYTE, the body a poison byte; `.b` is the Bucket view of the body
                                (count=P: P such regions side by side, `.bs`, for a call with P outputs)
    .read(want, what)           downloads the whole allocation once; every guard byte must be unchanged (the first changed
                                offset is named relative to the body), no body element may still hold the poison; returns
                                the body for the caller's own bit-for-bit comparison (.read_all: every body)
    .load(arrays)               for a bucket the call reads and writes: it holds values, and read(None) judges the guards
    guarded_runs(want, ...)     the one or two Guarded a case needs under the poison rule below
    launched(want, ...)         the loop over them around one launch, for a test's own comparison
    frozen(arrays, dtype)       inputs uploaded into guarded regions; .assert_intact() after the call

The poison rule is a condition, not a tolerance: in a run that counts, no element of `want` has the poison's bit
pattern, so "still the poison" means "not written" and nothing else. poisons_for(want) picks the first candidate byte
whose repeated pattern does not occur in `want` (raw bits: a NaN of `want` with the poison's own bits counts as an
occurrence, a NaN with other bits does not); if every candidate occurs (1-byte element types from about a thousand
elements on) it returns two bytes and the case runs once under each: an unwritten element can equal `want` under at
most one of the two. No element is ever left unjudged.

The logic works on host arrays (layout / image / check_image), so tests/test_guard_cpu.py proves it without a GPU; the
classes below add the upload and the one download.
"""
import numpy as np

from fmi_amd.device import _HOST_DTYPE, DType, dtype_of, storage_bytes

FRONT = 4096            # bytes of guard before the body (and before its slack)
TILE = 256 * 16         # one 256-lane tile of 16-B lane groups
BACK = 2 * TILE         # bytes of guard after the body: a one-tile overrun stays inside the allocation
GUARD_BYTE = 0xE7
CANDIDATES = (0xA5, 0x5A, 0xC3, 0x3C, 0x96)
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}

assert GUARD_BYTE not in CANDIDATES


def as_dtype(dtype) -> DType:
    return dtype if isinstance(dtype, DType) else dtype_of(dtype)


def element_bytes(dtype) -> int:
    """Bytes of one judged element: the storage element, or one byte (two nibbles) of the packed F4E2M1."""
    return np.dtype(_HOST_DTYPE[as_dtype(dtype)]).itemsize


def raw_elements(arr, dtype) -> np.ndarray:
    """`arr` (one array or a sequence of them) as the unsigned integers of its elements' raw bits, flattened. An
    F4E2M1 array is its packed bytes."""
    u = UINT[element_bytes(dtype)]
    parts = arr if isinstance(arr, (list, tuple)) else [arr]
    out = []
    for a in parts:
        a = np.ascontiguousarray(a)
        if a.dtype.itemsize != np.dtype(u).itemsize:
            raise ValueError(f"elements of {a.dtype} are not the {np.dtype(u).itemsize} bytes of {as_dtype(dtype).name}")
        out.append(a.reshape(-1).view(u))
    return np.concatenate(out) if out else np.empty(0, u)


def pattern(byte: int, dtype):
    """The poison element: `byte` repeated over one element, as an unsigned integer scalar."""
    size = element_bytes(dtype)
    return UINT[size](int.from_bytes(bytes([byte]) * size, "little"))


def occurs(byte: int, want, dtype) -> bool:
    """Whether any element of `want` has the poison's bit pattern (raw bits, NaNs included)."""
    return bool((raw_elements(want, dtype) == pattern(byte, dtype)).any())


def poisons_for(want, dtype, candidates=CANDIDATES) -> tuple:
    """(byte,) for the first candidate that does not occur in `want`, else the first two candidates: the case then runs
    under both."""
    for c in candidates:
        if not occurs(c, want, dtype):
            return (c,)
    if len(candidates) < 2 or candidates[0] == candidates[1]:
        raise ValueError("the two-run fallback needs two different candidate bytes")
    return (candidates[0], candidates[1])


class Layout:
    """Where the body sits in the allocation, in bytes. `n` elements at `offset` elements of slack."""

    def __init__(self, n: int, dtype, offset: int = 0, front: int = FRONT, back: int = BACK):
        self.dtype = as_dtype(dtype)
        self.n, self.offset = int(n), int(offset)
        if self.dtype == DType.F4E2M1 and self.offset % 2:
            raise ValueError("an F4E2M1 body starts on a byte: even element offsets only")
        self.front = front
        self.body = front + storage_bytes(self.dtype, self.offset)  # first byte of the body
        self.nbytes = storage_bytes(self.dtype, self.n)
        self.total = self.body + self.nbytes + back

    def shortened(self, n: int) -> "Layout":
        """The same allocation with the body declared `n` <= self.n elements long: what follows counts as guard."""
        if not 0 <= n <= self.n:
            raise ValueError("shortened: a declared body lies inside the real one")
        return Layout(n, self.dtype, self.offset, self.front, self.total - self.body - storage_bytes(self.dtype, n))


def image(lay: Layout, fill) -> np.ndarray:
    """The allocation's initial bytes: GUARD_BYTE everywhere but the body; the body `fill` (a poison byte, or the bytes of
    an input)."""
    raw = np.full(lay.total, GUARD_BYTE, np.uint8)
    raw[lay.body:lay.body + lay.nbytes] = fill
    return raw


def check_guards(raw: np.ndarray, lay: Layout, what: str = "") -> None:
    """Every byte outside the body still GUARD_BYTE, else AssertionError naming the first changed offset."""
    raw = np.asarray(raw, np.uint8)
    assert raw.size == lay.total, (what, raw.size, lay.total)
    end = lay.body + lay.nbytes
    bad = np.flatnonzero(raw != GUARD_BYTE)
    bad = bad[(bad < lay.body) | (bad >= end)]
    if bad.size:
        i = int(bad[0])
        where = f"body - {lay.body - i}" if i < lay.body else f"body + {i - lay.body} (output bytes + {i - end})"
        raise AssertionError(f"{what}: guard written: {bad.size} guard byte(s) changed, first at {where}: "
                             f"0x{int(raw[i]):02x}")


def check_image(raw: np.ndarray, lay: Layout, poison: int, want, what: str = "", paired: bool = False) -> np.ndarray:
    """The judgement of one run over the downloaded allocation `raw`: guards intact, no element left unwritten. Returns
    the body in the dtype's host type. `want` (the expected body, any shape; None = guards alone) must not hold the poison
    unless this run is one of a two-poison pair (`paired`): then the elements where it does are judged by the other run."""
    check_guards(raw, lay, what)
    host = np.dtype(_HOST_DTYPE[lay.dtype])
    body = np.asarray(raw, np.uint8)[lay.body:lay.body + lay.nbytes].copy().view(host)
    if want is None:
        return body
    got, w, pat = raw_elements(body, lay.dtype), raw_elements(want, lay.dtype), pattern(poison, lay.dtype)
    assert got.size == w.size, f"{what}: the body holds {got.size} elements, want {w.size}"
    judged = w != pat
    if not paired:
        assert judged.all(), (f"{what}: poison rule broken: want[{int(np.flatnonzero(~judged)[0])}] has the poison's bits "
                              f"0x{int(pat):x}; choose the byte with poisons_for(want)")
    stale = np.flatnonzero((got == pat) & judged)
    if stale.size:
        raise AssertionError(f"{what}: element {int(stale[0])} unwritten: {stale.size} of {got.size} element(s) still hold "
                             f"the poison 0x{int(pat):x}, last at {int(stale[-1])}")
    return body


def check_frozen(raw: np.ndarray, before: np.ndarray, lay: Layout, what: str = "") -> None:
    """An input's allocation after the call against what was uploaded: body and guards."""
    check_guards(raw, lay, what)
    diff = np.flatnonzero(np.asarray(raw, np.uint8) != before)
    if diff.size:
        i = int(diff[0]) - lay.body
        raise AssertionError(f"{what}: input modified: {diff.size} byte(s) changed, first at body + {i} (element "
                             f"{i // element_bytes(lay.dtype)}): 0x{int(before[diff[0]]):02x} -> 0x{int(raw[diff[0]]):02x}")


def host_bits(arr, dtype) -> np.ndarray:
    """`arr` flattened in the dtype's host type; bit patterns of the same element size (np.uint16 for F16) are viewed,
    never converted."""
    host = np.dtype(_HOST_DTYPE[as_dtype(dtype)])
    arr = np.ascontiguousarray(arr).reshape(-1)
    if arr.dtype == host:
        return arr
    if arr.dtype.itemsize != host.itemsize or arr.dtype.kind == "f" or host.kind not in "fiu":
        raise ValueError(f"{arr.dtype} values are not the raw bits of {as_dtype(dtype).name}")
    return arr.view(host)


# ---- on the device -----------------------------------------------------------------------------------------------------
class _Arena:
    """Regions (a Layout and its initial bytes each) side by side in ONE device allocation, each with guards of its
    own: one upload, one download, however many buckets a call takes."""

    def __init__(self, layouts, fills):
        from fmi_amd import Bucket

        self.stride = -(-max(lay.total for lay in layouts) // 256) * 256
        # a region runs to the next one: the padding behind its back guard is guard as well
        self.lays = [Layout(lay.n, lay.dtype, lay.offset, lay.front, self.stride - lay.body - lay.nbytes) for lay in layouts]
        self.before = np.concatenate([image(lay, fill) for lay, fill in zip(self.lays, fills)])
        self.whole = Bucket(self.before.size, DType.U8)
        assert self.whole.ptr % 256 == 0, "device allocations are at least 256-B aligned"
        self.whole.upload(self.before)
        self.bs = [Bucket(lay.n, lay.dtype, ptr=self.whole.ptr + j * self.stride + lay.body, owner=self.whole)
                   for j, lay in enumerate(self.lays)]

    def refill(self, fills=None) -> None:
        if fills is not None:
            self.before = np.concatenate([image(lay, fill) for lay, fill in zip(self.lays, fills)])
        self.whole.upload(self.before)

    def regions(self):
        """The one download, cut into (bytes now, bytes uploaded, layout) per region."""
        raw = self.whole.numpy()
        return [(raw[j * self.stride:(j + 1) * self.stride], self.before[j * self.stride:(j + 1) * self.stride], lay)
                for j, lay in enumerate(self.lays)]


class Guarded:
    """Outputs: `.b` is the poisoned body (`.bs`: `count` of them, for a call with several outputs), 16-B aligned at
    offset 0 and `offset` elements off alignment otherwise."""

    def __init__(self, n, dtype, offset=0, poison=CANDIDATES[0], paired=False, count=1):
        if poison == GUARD_BYTE and paired:
            raise ValueError("the guard byte is no poison of a two-run pair")
        self.poison, self.paired, self.count = int(poison), paired, count
        self.arena = _Arena([Layout(n, dtype, offset)] * count, [self.poison] * count)
        self.bs = self.arena.bs
        self.b = self.bs[0]

    def repoison(self, poison=None, paired=None) -> "Guarded":
        """Fill guards and bodies again before another launch into the same buckets."""
        if poison is not None:
            self.poison = int(poison)
        if paired is not None:
            self.paired = paired
        self.arena.refill([self.poison] * self.count)
        return self

    def load(self, arrays) -> "Guarded":
        """Bodies that the call reads AND writes (an inout operand, an in-place program, a folded amax word): they hold
        these values, not the poison, and read(None) judges the guards alone; what the call left in them is compared by
        the caller, where an element it skipped shows as its old value."""
        assert len(arrays) == self.count
        self.arena.refill([host_bits(a, self.arena.lays[0].dtype).view(np.uint8) for a in arrays])
        return self

    def read_all(self, wants, what="") -> list:
        """Every body, judged against wants[j] (None: guards alone)."""
        assert len(wants) == self.count
        return [check_image(raw, lay, self.poison, w, f"{what}: output {j}" if self.count > 1 else what, self.paired)
                for j, ((raw, _, lay), w) in enumerate(zip(self.arena.regions(), wants))]

    def read(self, want, what="", declared_n=None) -> np.ndarray:
        """The body of a single output. declared_n: judge against a body declared that many elements long (what follows
        it counts as guard)."""
        assert self.count == 1
        if declared_n is None:
            return self.read_all([want], what)[0]
        (raw, _, lay), = self.arena.regions()
        return check_image(raw, lay.shortened(declared_n), self.poison, want, what, self.paired)


def guarded_runs(want, n, dtype, offset=0, count=1):
    """The Guarded outputs a case needs, chosen on the CPU before any launch: one whose poison does not occur in
    `want`, or two with different poisons, the case running once into each. `want`: the expected body, or the sequence of
    the `count` bodies of one call (one poison for the group)."""
    ps = poisons_for(want, dtype)
    assert len(ps) == 2 or not occurs(ps[0], want, dtype)
    return [Guarded(n, dtype, offset, p, paired=len(ps) == 2, count=count) for p in ps]


def launched_all(wants, n, dtype, launch, what="", offset=0):
    """For a test's own comparison: `launch(buckets)` into len(wants) guarded, poisoned outputs, the device synchronised,
    guards and poison judged; yields the list of bodies, once, or once per poison of a pair:

        for got in launched_all(want, n, dtype, lambda bs: scan_peers(op, alg, bs, ins), what):
            for r in range(P): assert_bits(got[r], want[r], ...)"""
    from fmi_amd import sync

    wants = list(wants)
    for g in guarded_runs(wants, n, dtype, offset, len(wants)):
        launch(g.bs)
        sync()
        yield g.read_all(wants, what)


def launched(want, n, dtype, launch, what="", offset=0):
    """launched_all for a call with one output: `launch(bucket)`, yields the body."""
    for got in launched_all([want], n, dtype, lambda bs: launch(bs[0]), what, offset):
        yield got[0]


class FrozenSet:
    """Inputs a call must leave alone, each in a guarded region of its own. `.bs`: their buckets."""

    def __init__(self, arrays, dtype, offsets=0, n=None):
        dtype = as_dtype(dtype)
        offs = [offsets] * len(arrays) if isinstance(offsets, int) else list(offsets)
        bits = [host_bits(a, dtype) for a in arrays]
        # F4E2M1: n elements in (n + 1) // 2 packed bytes
        lays = [Layout(b.size if n is None else n, dtype, o) for b, o in zip(bits, offs)]
        self.arena = _Arena(lays, [b.view(np.uint8) for b in bits])
        self.bs = self.arena.bs

    def assert_intact(self, what="") -> None:
        for k, (raw, before, lay) in enumerate(self.arena.regions()):
            check_frozen(raw, before, lay, f"{what}: input {k}")


def frozen(arrays, dtype, offsets=0) -> FrozenSet:
    """Every array uploaded into a guarded region; offsets: one element offset for all, or one per array."""
    return FrozenSet(arrays, dtype, offsets)


