"""FMI_F8E4M3 / FMI_F8E5M2 on the MI355X: the packed pairwise combines on every pair of patterns, fmi_dev_convert on
the boundary set, the fused f32-accumulating P-way kernels, their fallback, the plain P-way programs (pairwise passes in
order), FMI_OP_AVG, graph capture, the communicator and the torch glue. Every comparison is on the raw bytes against
tests/_fp8.py (pinned to torch CPU by tests/test_fp8_cpu.py); a NaN matches any NaN, every other byte must be equal."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fmi_amd
from fmi_amd import Alg, Bucket, DType, Graph, Op, PinnedArray, Stream
from fmi_amd.comm import Path
from tests import _fp8 as F
from tests import _guard as G
from tests import _half as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"e4m3": DType.F8E4M3, "e5m2": DType.F8E5M2}
OP = {"sum": Op.SUM, "prod": Op.PROD, "max": Op.MAX, "min": Op.MIN}
N_FUSED = 8245  # 515 lane groups of 16 B: two whole 256-thread tiles, a partial tile of 3, and a 5-byte tail
N_PLAIN = 4099
FUSED_P = [2, 3, 5, 8, 13, 16]


def bucket(bits, kind, offset=0):
    """A device bucket holding these bytes, starting `offset` bytes past a 16-B boundary."""
    bits = np.asarray(bits, np.uint8)
    b = Bucket(bits.size + offset, DT[kind])
    b.upload(np.concatenate([np.zeros(offset, np.uint8), bits]))
    return b.view(offset, bits.size) if offset else b


def empty(n, kind, offset=0):
    b = Bucket(n + offset, DT[kind])
    return b.view(offset, n) if offset else b


def read(b):
    return b.numpy()


# ---- pairwise: every (a, b) of the 256 x 256 table ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(extra=0):
    a, b = F.table_pairs()
    if extra:  # a partial tile and a tail below 16 B: the table's first pairs again, swapped
        a, b = np.concatenate([a, b[1000:1000 + extra]]), np.concatenate([b, a[1000:1000 + extra]])
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def table_want(op, kind, extra=0):
    w = F.combine(op, *table(extra), kind)
    w.setflags(write=False)
    return w


@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("op", F.OPS)
def test_pairwise_every_pair_of_patterns(device, op, kind):
    """fmi_dev_reduce_pair on whole pair tiles (n = 65,536), with a partial tile and a < 16-B tail (n + 21), and on
    buckets 1 and 3 bytes past a 16-B boundary (the scalar kernel)."""
    for extra, off_a, off_b in ((0, 0, 0), (21, 0, 0), (0, 1, 1), (21, 3, 1)):
        a, b = table(extra)
        da, db = bucket(a, kind, off_a), bucket(b, kind, off_b)
        fmi_amd.reduce_pair(OP[op], da, db)
        fmi_amd.sync()
        tag = f"reduce_pair {kind} {op} n={a.size} offsets {off_a}/{off_b}"
        F.assert_bits(read(da), table_want(op, kind, extra), kind, tag)
        assert np.array_equal(read(db), b), f"{tag}: `in` was modified"


@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("op", F.OPS)
def test_combine_and_batch_every_pair_of_patterns(device, op, kind):
    a, b = table(21)
    want = table_want(op, kind, 21)
    da, db, out = bucket(a, kind), bucket(b, kind), empty(a.size, kind)
    fmi_amd.combine(OP[op], out, da, db)
    fmi_amd.sync()
    F.assert_bits(read(out), want, kind, f"combine {kind} {op}")
    # inout == in: op(a, a)
    fmi_amd.reduce_pair(OP[op], da, da)
    fmi_amd.sync()
    F.assert_bits(read(da), F.combine(op, a, a, kind), kind, f"reduce_pair inout == in {kind} {op}")
    # three descriptors in one batch, one of them empty
    h = 30000
    x0, y0, x1, y1 = bucket(a[:h], kind), bucket(b[:h], kind), bucket(a[h:], kind), bucket(b[h:], kind)
    fmi_amd.reduce_pair_batch(OP[op], [(x0, y0), (empty(0, kind), empty(0, kind)), (x1, y1)])
    fmi_amd.sync()
    F.assert_bits(np.concatenate([read(x0), read(x1)]), want, kind, f"reduce_pair_batch {kind} {op}")


@pytest.mark.parametrize("kind", F.KINDS)
def test_host_reduce_pair_every_pair_of_patterns(device, kind):
    a, b = table(21)
    for op in F.OPS:
        x, y = np.array(a), np.array(b)  # pageable: the staged pipeline
        fmi_amd.host_reduce_pair(OP[op], x, y, dtype=DT[kind])
        F.assert_bits(x, table_want(op, kind, 21), kind, f"host_reduce_pair pageable {kind} {op}")
    px, py = PinnedArray(a.size, np.uint8), PinnedArray(a.size, np.uint8)
    try:
        for op in F.OPS:  # page-locked: zero-copy
            px.array[:], py.array[:] = a, b
            fmi_amd.host_reduce_pair(OP[op], px.array, py.array, dtype=DT[kind])
            F.assert_bits(np.array(px.array), table_want(op, kind, 21), kind, f"host_reduce_pair pinned {kind} {op}")
    finally:
        px.free()
        py.free()


@pytest.mark.parametrize("kind", F.KINDS)
def test_pairwise_drops_the_flag_and_refuses_avg(device, kind):
    a, b = table()
    da, db = bucket(a, kind), bucket(b, kind)
    fmi_amd._lib.call("fmi_dev_reduce_pair", int(Op.SUM), int(DT[kind]) | fmi_amd.ACC_F32, da.ptr, db.ptr, a.size, None)
    fmi_amd.sync()
    F.assert_bits(read(da), table_want("sum", kind), kind, "reduce_pair with FMI_ACC_F32")
    with pytest.raises(fmi_amd.FmiError, match="FMI_ERR_INVALID.*FMI_OP_AVG"):
        fmi_amd.reduce_pair(Op.AVG, da, db)


@pytest.mark.parametrize("kind", F.KINDS)
def test_fill_synthetic(device, kind):
    n = 4099
    b = empty(n, kind).fill_synthetic(seed=77, peer=3)
    fmi_amd.sync()
    assert np.array_equal(read(b), F.synthetic(kind, n, 77, 3))
    b = empty(n, kind, 3).fill_synthetic(seed=77, peer=3, first=100)
    fmi_amd.sync()
    assert np.array_equal(read(b), F.synthetic(kind, n, 77, 3, start=100))
    with pytest.raises(fmi_amd.FmiError, match="FMI_ERR_INVALID"):
        fmi_amd._lib.call("fmi_dev_fill_synthetic", int(DT[kind]) | fmi_amd.ACC_F32, b.ptr, n, 1, 0, None)


# ---- fmi_dev_convert -----------------------------------------------------------------------------------------------
def raw_bucket(arr, dtype, offset=0):
    """A bucket of `dtype` holding the raw bits of `arr`, `offset` elements past a 16-B boundary."""
    arr = np.ascontiguousarray(arr)
    b = Bucket(arr.size + offset, dtype)
    b.upload(np.concatenate([np.zeros(offset, arr.dtype), arr]))
    return b.view(offset, arr.size) if offset else b


@pytest.mark.parametrize("kind", F.KINDS)
def test_convert_f32_boundary_set(device, kind):
    """The 393,216 boundary values: every rounding tie of the format with its two f32 neighbours, every overflow
    threshold, every subnormal boundary, +-0, +-inf, NaNs. Aligned (8 elements per thread) and unaligned (scalar)."""
    x = F.boundary_f32()
    want = F.narrow(x, kind)
    src, dst = raw_bucket(x, np.float32), empty(x.size, kind)
    fmi_amd.convert(dst, src)
    fmi_amd.sync()
    F.assert_bits(read(dst), want, kind, f"convert f32 -> {kind}")
    m = 40000 + 13
    src, dst = raw_bucket(x[:m], np.float32, 1), empty(m, kind, 3)
    fmi_amd.convert(dst, src)
    fmi_amd.sync()
    F.assert_bits(read(dst), want[:m], kind, f"convert f32 -> {kind}, unaligned")


@pytest.mark.parametrize("kind", F.KINDS)
def test_convert_widens_all_patterns(device, kind):
    bits = np.tile(np.arange(256, dtype=np.uint8), 5)[:1275]  # whole groups of 8 (to f32) or 16 (to the 16-bit floats) and a tail
    want = F.widen(bits, kind)
    for off in (0, 1):
        dst = Bucket(bits.size + off, np.float32).view(off, bits.size)
        fmi_amd.convert(dst, bucket(bits, kind, off))
        fmi_amd.sync()
        got = dst.numpy()
        assert np.all((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))), (kind, off)
    # to the 16-bit floats: e5m2 is exact in both, e4m3 in both as well (4 significant bits, exponents -9..8)
    for hk, hd in (("f16", DType.F16), ("bf16", DType.BF16)):
        dst = Bucket(bits.size, hd)
        fmi_amd.convert(dst, bucket(bits, kind))
        fmi_amd.sync()
        H.assert_bits(dst.numpy().view(np.uint16), H.narrow(want, hk), hk, "sum", f"convert {kind} -> {hk}")


@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("hk,hd", [("f16", DType.F16), ("bf16", DType.BF16)])
def test_convert_narrows_every_16bit_pattern(device, hk, hd, kind):
    bits = np.arange(65536, dtype=np.uint16)
    src, dst = raw_bucket(bits if hk == "bf16" else bits.view(np.float16), hd), empty(bits.size, kind)
    fmi_amd.convert(dst, src)
    fmi_amd.sync()
    F.assert_bits(read(dst), F.narrow(H.widen(bits, hk), kind), kind, f"convert {hk} -> {kind}")


def test_convert_in_place_copy_and_between_the_two(device):
    bits = np.tile(np.arange(256, dtype=np.uint8), 9)[:2061]
    for off in (0, 5):
        # e4m3 -> e5m2 in place (equal element size), and back out of place
        b = bucket(bits, "e4m3", off)
        as5 = Bucket(bits.size, DType.F8E5M2, ptr=b.ptr)
        fmi_amd.convert(as5, b)
        fmi_amd.sync()
        want5 = F.narrow(F.widen(bits, "e4m3"), "e5m2")
        F.assert_bits(read(as5), want5, "e5m2", f"convert e4m3 -> e5m2 in place, offset {off}")
        back = empty(bits.size, "e4m3", off)
        fmi_amd.convert(back, as5)
        fmi_amd.sync()
        F.assert_bits(read(back), F.narrow(F.widen(want5, "e5m2"), "e4m3"), "e4m3", f"convert e5m2 -> e4m3, offset {off}")
        # equal dtypes: a copy of the bits, NaN payloads and all; dst == src is allowed
        c = empty(bits.size, "e5m2", off)
        fmi_amd.convert(c, bucket(bits, "e5m2"))
        fmi_amd.convert(c, c)
        fmi_amd.sync()
        assert np.array_equal(read(c), bits)
    x = F.boundary_f32()[:4099]
    c = Bucket(x.size, np.float32)
    fmi_amd.convert(c, raw_bucket(x, np.float32))
    fmi_amd.sync()
    assert np.array_equal(c.numpy().view(np.uint32), x.view(np.uint32))
    with pytest.raises(fmi_amd.FmiError, match="FMI_ERR_INVALID.*fmi_dev_convert"):
        fmi_amd.convert(Bucket(8, np.float64), c, n=8)


# ---- the fused f32-accumulating kernels ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def peer_bits(src, kind, n, P, seed):
    if src == "cancel":
        xs = F.cancel_inputs(kind, n, P, seed)
    elif src == "overflow":
        xs = F.overflow_inputs(kind, n, P, seed)
    elif src == "order":
        xs = F.order_inputs(kind, n, P, seed)
    elif src == "unit":  # magnitudes in [0.5, 2), either sign: products of 8 stay in range, every significand occurs
        rng = np.random.default_rng(seed)
        lo, span = (0x30, 16) if kind == "e4m3" else (0x38, 8)
        xs = [(lo + rng.integers(0, span, n) + 0x80 * rng.integers(0, 2, n)).astype(np.uint8) for _ in range(P)]
    elif src == "zeros":  # synthetic values with +-0 seeded in, differently per peer
        xs = [F.synthetic(kind, n, seed, p) for p in range(P)]
        for p, x in enumerate(xs):
            x[(np.arange(n) + p) % 5 == 0] = (0x00, 0x80)[p % 2]
    elif src == "signed":  # synthetic values with +-0 and NaN seeded in, differently per peer: max / min depend on the rank
        xs = [F.synthetic(kind, n, seed, p) for p in range(P)]
        nan = 0x7F if kind == "e4m3" else 0x7E
        for p, x in enumerate(xs):
            x[(np.arange(n) + p) % 5 == 0] = (0x00, 0x80)[p % 2]
            x[(np.arange(n) + 3 * p) % 11 == 0] = nan | (0x80 if p % 3 == 0 else 0)
    else:
        xs = [F.synthetic(kind, n, seed, p) for p in range(P)]
    for x in xs:
        x.setflags(write=False)
    return tuple(xs)


@functools.lru_cache(maxsize=None)
def want_acc(family, src, kind, op, n, P, seed, root=0):
    w = F.expected_acc(family, kind, op, list(peer_bits(src, kind, n, P, seed)), root)
    if src == "synthetic":  # at most 1 % of the expected elements may be NaN, so that the comparison is on bytes
        for x in ([w] if isinstance(w, np.ndarray) else w[1] + [w[0]] if family == "reduce" else w):
            assert F.is_nan(x, kind).mean() <= 0.01, (family, src, kind, op, P)
    return w


@functools.lru_cache(maxsize=None)
def want_plain(family, src, kind, op, n, P, seed, root=0):
    return F.expected_plain(family, kind, op, list(peer_bits(src, kind, n, P, seed)), root)


def upload(src, kind, n, P, seed, offset=0):
    return [bucket(x, kind, offset) for x in peer_bits(src, kind, n, P, seed)]


def check_trees(want, src, kind, op, n, P, seed, acc, roots=None, ranks=None, offset=0, what=""):
    ins = upload(src, kind, n, P, seed, offset)
    tag = f"{what}{src} {kind} {op} P={P} n={n} acc={acc}"

    def check(alg, w, rank, name):
        """One call into a guarded, poisoned output `offset` bytes off alignment (tests/_guard.py), compared on its bytes."""
        for got in G.launched(w, n, DT[kind], lambda out: fmi_amd.reduce_tree(OP[op], alg, out, ins, rank=rank, accumulate_f32=acc),
                              name, offset):
            F.assert_bits(got, w, kind, name)

    for r in (sorted({0, 1, P - 1}) if ranks is None else ranks):
        check(Alg.ALLREDUCE, want("allreduce", src, kind, op, n, P, seed)[r], r, f"allreduce {tag} rank {r}")
    for root in (sorted({0, P - 1}) if roots is None else roots):
        check(Alg.REDUCE, want("reduce", src, kind, op, n, P, seed, root)[0], root, f"reduce {tag} root {root}")
    check(Alg.REDUCE_LTR, want("reduce_ltr", src, kind, op, n, P, seed), 0, f"reduce_ltr {tag}")


def check_scans(want, src, kind, op, n, P, seed, acc, offset=0, what=""):
    for alg, family in ((Alg.SCAN, "scan"), (Alg.SCAN_LTR, "scan_ltr")):
        ins, w = upload(src, kind, n, P, seed, offset), want(family, src, kind, op, n, P, seed)
        tag = f"{what}{family} {src} {kind} {op} P={P} n={n} acc={acc}"
        # every output guarded and poisoned (tests/_guard.py)
        for got in G.launched_all(w, n, DT[kind], lambda outs: fmi_amd.scan_peers(OP[op], alg, outs, ins, accumulate_f32=acc), tag, offset):
            for r in range(P):
                F.assert_bits(got[r], w[r], kind, f"{tag} output {r}")


@pytest.mark.parametrize("P", FUSED_P)
@pytest.mark.parametrize("kind", F.KINDS)
def test_fused_acc32(device, kind, P):
    """All five algorithms, SUM and PROD; every root of REDUCE at P = 5."""
    for op in ("sum", "prod"):
        check_trees(want_acc, "synthetic", kind, op, N_FUSED, P, 31, True, roots=range(P) if P == 5 else None)
        check_scans(want_acc, "synthetic", kind, op, N_FUSED, P, 31, True)


@pytest.mark.parametrize("kind", F.KINDS)
def test_fused_acc32_cancelling_inputs(device, kind):
    """Inputs on which the ALLREDUCE and REDUCE_LTR expectations differ, so that a wrong bracketing cannot hide behind
    the final rounding. e5m2: SUM, a large pair that cancels (absorption in f32). e4m3: an f32 SUM of e4m3 values is
    exact in every order (tests/_fp8.py::cancel_inputs), so its case is a PROD at P = 16 that differs through the f32
    range (tests/_fp8.py::order_inputs: left to right 448^15 is inf and inf x 0 is NaN, the trees end with +-0); the
    SUM inputs still run on it and tell f32 accumulation from per-combine rounding."""
    differing = lambda a, b: (~((a == b) | (F.is_nan(a, kind) & F.is_nan(b, kind)))).mean()  # noqa: E731
    P, seed = 8, 41
    a, b = want_acc("allreduce", "cancel", kind, "sum", N_FUSED, P, seed)[0], want_acc("reduce_ltr", "cancel", kind, "sum", N_FUSED, P, seed)
    if kind == "e5m2":
        assert differing(a, b) > 0.3
    else:
        assert (a != want_plain("allreduce", "cancel", kind, "sum", N_FUSED, P, seed)[0]).mean() > 0.5
    check_trees(want_acc, "cancel", kind, "sum", N_FUSED, P, seed, True)
    check_scans(want_acc, "cancel", kind, "sum", N_FUSED, P, seed, True)
    # PROD through the f32 range, both formats: three elements in four differ by construction
    P, seed = 16, 42
    a, b = want_acc("allreduce", "order", kind, "prod", N_FUSED, P, seed)[0], want_acc("reduce_ltr", "order", kind, "prod", N_FUSED, P, seed)
    assert differing(a, b) > 0.7
    check_trees(want_acc, "order", kind, "prod", N_FUSED, P, seed, True, ranks=[0, 7, 15], roots=[0, 5, 15])
    check_scans(want_acc, "order", kind, "prod", N_FUSED, P, seed, True)


@pytest.mark.parametrize("kind", F.KINDS)
def test_fused_acc32_overflowing_partials(device, kind):
    """Partial sums above 448 / 57344 that come back in range: with f32 accumulation the result is finite and small;
    the plain dtype (narrowed after every combine, not saturating) shows the overflow as NaN / inf."""
    P, seed = 8, 43
    w = want_acc("reduce_ltr", "overflow", kind, "sum", N_FUSED, P, seed)
    assert not F.is_nan(w, kind).any() and np.abs(F.widen(w, kind)).max() < 8
    check_trees(want_acc, "overflow", kind, "sum", N_FUSED, P, seed, True)
    p = want_plain("reduce_ltr", "overflow", kind, "sum", N_PLAIN, P, seed)
    assert (F.is_nan(p, kind) | np.isinf(F.widen(p, kind))).all()
    check_trees(want_plain, "overflow", kind, "sum", N_PLAIN, P, seed, False, ranks=[0], roots=[0])


# ---- the fallback: widen, the FMI_F32 program, narrow ------------------------------------------------------------
@pytest.mark.parametrize("P", [17, 33])
@pytest.mark.parametrize("kind", F.KINDS)
def test_acc32_fallback_beyond_sixteen_peers(device, kind, P):
    check_trees(want_acc, "cancel", kind, "sum", 2061, P, 44, True, what="fallback ")
    check_scans(want_acc, "synthetic", kind, "sum", 2061, P, 44, True, what="fallback ")


@pytest.mark.parametrize("kind", F.KINDS)
def test_acc32_fallback_unaligned(device, kind):
    check_trees(want_acc, "cancel", kind, "sum", 2061, 5, 45, True, offset=1, what="unaligned ")
    check_scans(want_acc, "synthetic", kind, "prod", 2061, 5, 45, True, offset=3, what="unaligned ")


# ---- plain P-way programs: pairwise passes in the program's order -------------------------------------------------
@pytest.mark.parametrize("P", [3, 5, 8, 17])
@pytest.mark.parametrize("kind", F.KINDS)
def test_plain_programs(device, kind, P):
    """Narrowed after every combine, in the program's own order, at all five algorithms."""
    check_trees(want_plain, "synthetic", kind, "sum", N_PLAIN, P, 51, False)
    check_scans(want_plain, "synthetic", kind, "sum", N_PLAIN, P, 51, False)
    check_trees(want_plain, "cancel", kind, "sum", N_PLAIN, P, 52, False, ranks=[P - 1], roots=[1])
    check_trees(want_plain, "unit" if P <= 8 else "zeros", kind, "prod", N_PLAIN, P, 53, False, ranks=[1], roots=[P - 1])


@pytest.mark.parametrize("P", [3, 5, 8, 17])
@pytest.mark.parametrize("kind", F.KINDS)
def test_plain_max_min_every_rank(device, kind, P):
    """MAX / MIN keep an operand's byte: on +-0 and NaN every rank of an ALLREDUCE ends with its own bits (compared raw:
    selections make no NaN of their own). With the flag the same plain program runs."""
    src, seed = "signed", 54
    ins, out = upload(src, kind, N_PLAIN, P, seed), empty(N_PLAIN, kind)
    for op in ("max", "min"):
        w = want_plain("allreduce", src, kind, op, N_PLAIN, P, seed)
        assert any(not np.array_equal(w[0], w[r]) for r in range(1, P)), "the ranks' expectations should differ"
        for r in range(P):
            fmi_amd.reduce_tree(OP[op], Alg.ALLREDUCE, out, ins, rank=r, accumulate_f32=(r % 2 == 1))
            fmi_amd.sync()
            assert np.array_equal(read(out), w[r]), f"allreduce {op} {kind} P={P} rank {r}"
    check_scans(want_plain, src, kind, "max", N_PLAIN, P, seed, False)


# ---- FMI_OP_AVG ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [3, 8, 16, 17])
@pytest.mark.parametrize("kind", F.KINDS)
def test_avg(device, kind, P):
    """narrow(fl32(S x fl32(1 / P))): S the plain SUM result (widened) or, with the flag, the f32 program value."""
    n, seed = 2061, 61
    xs = list(peer_bits("cancel", kind, n, P, seed))
    ins, out = upload("cancel", kind, n, P, seed), empty(n, kind)
    for acc in (False, True):
        values = F.acc_values if acc else None
        for alg, family, rank in ((Alg.ALLREDUCE, "allreduce", P - 1), (Alg.REDUCE, "reduce", 1), (Alg.REDUCE_LTR, "reduce_ltr", 0)):
            if acc:
                s = values(family, kind, "sum", xs, rank if family == "reduce" else 0)
                s = s[rank] if family == "allreduce" else s[0] if family == "reduce" else s
            else:
                s = want_plain(family, "cancel", kind, "sum", n, P, seed, rank if family == "reduce" else 0)
                s = F.widen(s[rank] if family == "allreduce" else s[0] if family == "reduce" else s, kind)
            fmi_amd.reduce_tree(Op.AVG, alg, out, ins, rank=rank, accumulate_f32=acc)
            fmi_amd.sync()
            F.assert_bits(read(out), F.mean_of(s, P, kind), kind, f"avg {family} {kind} P={P} acc={acc}")
    with pytest.raises(fmi_amd.FmiError, match="FMI_ERR_INVALID.*FMI_OP_AVG"):
        fmi_amd.scan_peers(Op.AVG, Alg.SCAN, [empty(n, kind) for _ in range(P)], ins)


@pytest.mark.parametrize("kind", F.KINDS)
def test_mean_scale(device, kind):
    bits = np.tile(np.arange(256, dtype=np.uint8), 9)[:2061]
    want = F.mean_of(F.widen(bits, kind), 3, kind)
    for off in (0, 3):
        b = bucket(bits, kind, off)
        fmi_amd.mean_scale(b, 3)
        fmi_amd.sync()
        F.assert_bits(read(b), want, kind, f"mean_scale {kind} P=3 offset {off}")
    b = bucket(bits, kind)
    fmi_amd.mean_scale(b, 1)
    fmi_amd.sync()
    assert np.array_equal(read(b), bits)


# ---- graph capture ---------------------------------------------------------------------------------------------
def test_graph_capture(device):
    """One f32-accumulating ALLREDUCE at P = 8 (one fused kernel) is captured on a stream of its own and replayed
    twice: the same bits both times."""
    kind, n, P, seed = "e4m3", N_FUSED, 8, 71
    ins, out = upload("cancel", kind, n, P, seed), empty(n, kind)
    fmi_amd.sync()
    st = Stream()
    g = Graph.capture(st, lambda: fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, out, ins, rank=3, stream=st, accumulate_f32=True))
    try:
        got = []
        for _ in range(2):
            fmi_amd._lib.call("fmi_dev_memset_async", out.ptr, 0x55, out.nbytes, st.handle)
            g.launch(st)
            st.sync()
            got.append(read(out))
        assert np.array_equal(got[0], got[1])
        F.assert_bits(got[0], want_acc("allreduce", "cancel", kind, "sum", n, P, seed)[3], kind, "graph replay")
    finally:
        g.destroy()
        st.destroy()


# ---- the communicator: LOCAL transport, every rank compared -----------------------------------------------------
COMM_N = 3 * 4096 + 7


@pytest.mark.parametrize("N", [2, 3, 8])
@pytest.mark.parametrize("kind", F.KINDS)
def test_comm_collectives(device, N, kind):
    from tests.test_gpu_comm import run_ranks

    n, seed, src, root = COMM_N, 81, "cancel", N - 1
    xs, us = peer_bits(src, kind, n, N, seed), peer_bits("unit", kind, n, N, seed)

    def body(c, r):
        new = lambda: empty(n, kind)  # noqa: E731
        s = bucket(xs[r], kind)
        res = {}
        for acc in (False, True):
            ar, avg, red, sc = new(), new(), new(), new()
            c.allreduce(Op.SUM, s, ar, path=Path.TREE, accumulate_f32=acc)
            c.allreduce(Op.AVG, s, avg, path=Path.TREE, accumulate_f32=acc)
            c.reduce(Op.SUM, s, red if r == root else None, root, accumulate_f32=acc)
            c.scan(Op.SUM, s, sc, accumulate_f32=acc)
            fmi_amd.sync()
            res[acc] = (read(ar), read(avg), read(red) if r == root else None, read(sc))
        mx = new()
        c.allreduce(Op.MAX, s, mx)
        s2, o2 = bucket(xs[r], kind), new()
        c.reduce(Op.SUM, s2, o2 if r == root else None, root, sendbuf_partials=True, accumulate_f32=True)
        s3, o3 = bucket(us[r], kind), new()
        c.reduce(Op.PROD, s3, o3 if r == root else None, root, sendbuf_partials=True, accumulate_f32=True)
        fmi_amd.sync()
        res["max"], res["partial"], res["partial_prod"] = read(mx), read(s2), read(s3)
        res["root_prod"] = read(o3) if r == root else None
        if r == 0:
            with pytest.raises(fmi_amd.FmiError, match="FMI_ERR_UNSUPPORTED.*RCCL"):
                c.allreduce(Op.SUM, s, new(), path=Path.RCCL)
            with pytest.raises(fmi_amd.FmiError, match="FMI_ERR_UNSUPPORTED.*RCCL"):
                c.allreduce(Op.SUM, s, new(), path=Path.RCCL, accumulate_f32=True)
        return res

    res = run_ranks(N, body)
    l = list(xs)
    for acc in (False, True):
        want = want_acc if acc else want_plain
        w_ar, w_sc = want("allreduce", src, kind, "sum", n, N, seed), want("scan", src, kind, "sum", n, N, seed)
        w_red = want("reduce", src, kind, "sum", n, N, seed, root)[0]
        s_ar = F.acc_values("allreduce", kind, "sum", l) if acc else [F.widen(x, kind) for x in w_ar]
        for r in range(N):
            tag = f"{kind} N={N} acc={acc} rank {r}"
            F.assert_bits(res[r][acc][0], w_ar[r], kind, f"allreduce TREE {tag}")
            F.assert_bits(res[r][acc][1], F.mean_of(s_ar[r], N, kind), kind, f"allreduce AVG {tag}")
            F.assert_bits(res[r][acc][3], w_sc[r], kind, f"scan {tag}")
        F.assert_bits(res[root][acc][2], w_red, kind, f"reduce {kind} N={N} acc={acc} root {root}")
    w_mx = want_plain("allreduce", src, kind, "max", n, N, seed)
    w_sends = want_acc("reduce", src, kind, "sum", n, N, seed, root)[1]
    w_prod, w_prod_sends = want_acc("reduce", "unit", kind, "prod", n, N, seed, root)
    F.assert_bits(res[root]["root_prod"], w_prod, kind, f"reduce_sendbuf PROD {kind} N={N} root {root}")
    for r in range(N):
        assert np.array_equal(res[r]["max"], w_mx[r]), f"allreduce MAX {kind} N={N} rank {r}"
        F.assert_bits(res[r]["partial"], w_sends[r], kind, f"reduce_sendbuf {kind} N={N}: sendbuf of rank {r}")
        F.assert_bits(res[r]["partial_prod"], w_prod_sends[r], kind, f"reduce_sendbuf PROD {kind} N={N}: sendbuf of rank {r}")


@pytest.mark.parametrize("kind", F.KINDS)
def test_comm_allreduce_host(device, kind):
    from tests.test_gpu_comm import run_ranks

    N, n, seed = 2, COMM_N, 82
    xs = peer_bits("cancel", kind, n, N, seed)

    def body(c, r):
        out, out_acc = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        c.allreduce_host(Op.SUM, np.array(xs[r]), out, chunk=3 * 1024, dtype=DT[kind])
        c.allreduce_host(Op.SUM, np.array(xs[r]), out_acc, chunk=3 * 1024, accumulate_f32=True, dtype=DT[kind])
        return out, out_acc

    res = run_ranks(N, body)
    for r in range(N):
        F.assert_bits(res[r][0], want_plain("allreduce", "cancel", kind, "sum", n, N, seed)[r], kind, f"allreduce_host rank {r}")
        F.assert_bits(res[r][1], want_acc("allreduce", "cancel", kind, "sum", n, N, seed)[r], kind, f"allreduce_host acc rank {r}")


def test_comm_proc_transport(device, tmp_path):
    """Two ranks as two processes (PROC transport: shared-memory staging) on 8-bit float buckets."""
    from fmi_amd.comm import Transport, unique_id
    from tests._fp8_proc_worker import N_ELEMS, SEED

    N = 2
    uid = unique_id(Transport.PROC).hex()
    paths = [str(tmp_path / f"rank{r}.npz") for r in range(N)]
    procs = [subprocess.Popen([sys.executable, "-m", "tests._fp8_proc_worker", uid, str(N), str(r), paths[r]], cwd=ROOT,
                              env=dict(os.environ, FMI_PROC_TIMEOUT_S="90")) for r in range(N)]
    codes = []
    for p in procs:
        try:
            codes.append(p.wait(timeout=240))
        except subprocess.TimeoutExpired:
            p.kill()
            codes.append(p.wait())
    assert codes == [0] * N, f"rank exit codes {codes}"
    res = [dict(np.load(p)) for p in paths]
    for kind in F.KINDS:
        w_acc = want_acc("allreduce", "cancel", kind, "sum", N_ELEMS, N, SEED)
        w_max = want_plain("allreduce", "cancel", kind, "max", N_ELEMS, N, SEED)
        for r in range(N):
            F.assert_bits(res[r][f"{kind}_acc_sum"], w_acc[r], kind, f"PROC allreduce acc32 {kind} rank {r}")
            assert np.array_equal(res[r][f"{kind}_max"], w_max[r]), f"PROC allreduce max {kind} rank {r}"


# ---- the torch glue ---------------------------------------------------------------------------------------------
def test_torch_glue(device):
    """fmi_amd.collectives on torch.float8_e4m3fn device tensors (a child process: torch must be loaded before the
    library) equals the ctypes path and the definition."""
    r = subprocess.run([sys.executable, "-u", "-m", "tests._fp8_torch_worker"], cwd=ROOT, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0 and "fp8 torch glue ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_cpp_fp8_gpu(device):
    """Dev::convert and a pairwise combine on Dev::Bucket<Dev::float8_e4m3 / float8_e5m2> equal the host types' own
    narrowing and operator+ (fmi_amd/cpp/tests/test_fp8.cpp --gpu)."""
    exe = os.path.join(ROOT, "build", "cpp", "test_fp8")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fmi_amd", "cpp")], check=True)
    out = subprocess.run([exe, "--gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    assert "0 failed checks" in out.stderr
