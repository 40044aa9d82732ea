"""MXFP4 on the GPU (FMI_F4E2M1 in fmi_dev_reduce_tree_mx, fmi_dev_mx_quantize, fmi_dev_mx_dequantize and
fmi_comm_allreduce_mx), bit for bit against tests/_mxfp4.py: E2M1 codes and scale bytes exactly, an f32 output on its
uint32 view (a NaN matching any NaN). Scale arrays sit at odd addresses. Every output is pre-filled with other bytes and
sits inside a larger allocation: the bytes after it must come back unchanged, and an odd bucket's last high nibble 0."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fmi_amd
from fmi_amd import Alg, Bucket, DType, Graph, Op, Stream, Tune
from tests import _fp8 as F
from tests import _half as H
from tests import _mx as MX
from tests import _mxfp4 as M
from tests.test_gpu_fp8_scaled import N_FUSED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F4 = DType.F4E2M1
OP = {"sum": Op.SUM, "avg": Op.AVG}
N_TILE = M.N_TILE  # 256 * 32 + 96 + 17: one whole tile of blocks, three more blocks, an odd ragged block of 17
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, N_TILE, N_FUSED)
THREE_SIZES = (33, N_TILE, N_FUSED)
RANGES = ((112, 142), (120, 134))
ALGS = {
    "allreduce": ("allreduce", Alg.ALLREDUCE, lambda P: 0),
    "reduce_rootlast": ("reduce", Alg.REDUCE, lambda P: P - 1),
    "reduce_ltr": ("reduce_ltr", Alg.REDUCE_LTR, lambda P: 0),
}
GUARD = 32  # bytes after every output that must not change
FILL, SFILL, GFILL = 0x55, 0x11, 0xA7


@functools.lru_cache(maxsize=None)
def inputs(P, rng=M.ORDER_RANGE, n=N_FUSED, seed=None):
    """All 16 nibbles, per-block scales per peer from the range. The default (scale bytes 112..142, no seed) is
    M.order_inputs(P, n): the order cases. cut() of it to N_TILE or 33 is M.order_inputs(P, N_TILE) or (P, 33), the data
    tests/test_mxfp4_cpu.py asserts the bracketings to differ on, because a generator's shorter bucket is a prefix of
    its longer one. Shared and never modified."""
    xs, es = M.order_inputs(P, n) if seed is None and rng == M.ORDER_RANGE else M.random_inputs(n, P, 1000 + P if seed is None else seed, *rng)
    for a in xs + es:
        a.setflags(write=False)
    return tuple(xs), tuple(es)


def cut(xs, es, n):
    return [x[:n] for x in xs], [e[:MX.blocks(n)] for e in es]


def bytes_bucket(raw, dtype, offset=0, n=None):
    """`raw` bytes at `offset` bytes into an allocation; n: the element count (F4E2M1), default one per byte."""
    raw = np.asarray(raw, np.uint8)
    b = Bucket(raw.size + offset, DType.U8)
    b.upload(np.concatenate([np.zeros(offset, np.uint8), raw]))
    return Bucket(raw.size if n is None else n, dtype, ptr=b.ptr + offset, owner=b)


def fp4_bucket(codes, offset=0):
    return bytes_bucket(M.pack(codes), F4, offset, n=len(codes))


class Out:
    """The result and its scales inside guarded allocations. offset: bytes off 16-B alignment."""

    def __init__(self, n, out, offset=0):
        self.n, self.out = n, out
        self.nbytes = 4 * n if out == "f32" else (n + 1) // 2
        fill = np.full(n, 1.5, np.float32).view(np.uint8) if out == "f32" else np.full(self.nbytes, FILL, np.uint8)
        self.whole = bytes_bucket(np.concatenate([fill, np.full(GUARD, GFILL, np.uint8)]), DType.U8, offset)
        self.b = Bucket(n, DType.F32 if out == "f32" else F4, ptr=self.whole.ptr, owner=self.whole)
        self.sc = None
        if out != "f32":
            self.swhole = bytes_bucket(np.concatenate([np.full(MX.blocks(n), SFILL, np.uint8), np.full(GUARD, GFILL, np.uint8)]), DType.U8, 1)
            self.sc = Bucket(MX.blocks(n), DType.F8E8M0, ptr=self.swhole.ptr, owner=self.swhole)

    def read(self, what=""):
        raw = self.whole.numpy()
        assert (raw[self.nbytes:] == GFILL).all(), f"{what}: bytes after the output were written"
        if self.out == "f32":
            return raw[:self.nbytes].copy().view(np.float32), None
        sraw = self.swhole.numpy()
        assert (sraw[MX.blocks(self.n):] == GFILL).all(), f"{what}: bytes after the output scales were written"
        if self.n % 2:
            assert raw[self.nbytes - 1] >> 4 == 0, f"{what}: the last byte's unused high nibble is {raw[self.nbytes - 1] >> 4:#x}, not 0"
        return M.unpack(raw[:self.nbytes], self.n), sraw[:MX.blocks(self.n)].copy()


def run(alg, xs, es, op, out, root=0, offset=0, stream=None, what=""):
    n = xs[0].size
    ins = [fp4_bucket(x, offset) for x in xs]
    scs = [bytes_bucket(e, DType.F8E8M0, 1) for e in es]
    o = Out(n, out, offset)
    fmi_amd.reduce_tree_mx(OP[op], alg, o.b, o.sc, ins, scs, rank=root, stream=stream)
    fmi_amd.sync()
    return o.read(what)


def check(name, xs, es, op, out, offset=0, what=""):
    family, alg, root_of = ALGS[name]
    root = root_of(len(xs))
    what = f"{what} {name} {op} P={len(xs)} n={xs[0].size} out={out}"
    want, want_sc = M.expected(family, xs, es, op, out, root)
    got, got_sc = run(alg, xs, es, op, out, root, offset, what=what)
    M.assert_mx(got, got_sc, want, want_sc, out, what)
    return got, got_sc


# ---- 1. the fused kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["same", "f32"])
@pytest.mark.parametrize("P", [2, 3, 8, 16])
@pytest.mark.parametrize("name", list(ALGS))
def test_fused(device, name, P, out):
    """The f32 output at scale bytes 112..142 pins the order of the sum (tests/test_mxfp4_cpu.py measures how often the
    bracketings differ there); the E2M1 output the block amax, the scale byte and the narrowing. SUM everywhere, the mean
    at P = 3 and 8."""
    for rng in RANGES:
        xs, es = inputs(P, rng)
        for n in THREE_SIZES:
            for op in (("sum", "avg") if P in (3, 8) else ("sum",)):
                check(name, *cut(xs, es, n), op, out, what=f"scales {rng}")


@pytest.mark.parametrize("out", ["same", "f32"])
def test_fused_every_size(device, out):
    """P = 8: nothing but a ragged block (1, 2, 31), one block (32), a block and a ragged one (33, 63), two blocks (64),
    two and one element (65), more than a tile with an odd tail, N_FUSED."""
    xs, es = inputs(8)
    for n in SIZES:
        for name in ALGS:
            check(name, *cut(xs, es, n), "sum", out)
        check("allreduce", *cut(xs, es, n), "avg", out)


@pytest.mark.parametrize("policy", [0, 2])
def test_fused_both_access_policies(device, policy):
    before = fmi_amd.tune_get(Tune.FUSED_POLICY)
    fmi_amd.tune_set(Tune.FUSED_POLICY, policy)
    try:
        for P in (3, 8):
            xs, es = inputs(P)
            for n in (N_TILE, N_FUSED):
                for out in ("same", "f32"):
                    check("allreduce", *cut(xs, es, n), "sum", out, what=f"policy {policy}")
    finally:
        fmi_amd.tune_set(Tune.FUSED_POLICY, before)


# ---- 2. decided blocks -----------------------------------------------------------------------------------------------
# block 0, block 257 (the second 256-lane tile), the ragged last block 259 (17 elements)
PLACES = (0, 257, 259)
NEIGHBOURS = (1, 256, 258)


def _base(P=3):
    xs, es = cut(*inputs(P, (120, 134)), N_TILE)
    return [x.copy() for x in xs], [e.copy() for e in es]


def _span(b, n=N_TILE):
    return slice(32 * b, min(32 * b + 32, n))


def test_decided_blocks(device):
    cases = {}

    def case(name, edit, want_e, want_q=None, P=3):
        xs, es = _base(P)
        for b in PLACES:
            edit(xs, es, b)
        cases[name] = (xs, es, want_e, want_q)

    def single(k, codes):
        """The block is zero but for peer p's element 5 = codes[p], every scale 2^k."""
        def edit(xs, es, b):
            for x, e in zip(xs, es):
                x[_span(b)] = 0
                e[b] = 127 + k
            for p, c in enumerate(codes):
                xs[p][_span(b).start + 5] = c
        return edit

    # 6 = 1.5 * 2^2 sits ON the threshold mantissa 0x400000: e_out = 127 + k + 2 - 2, the element stays 6 (code 7)
    case("the maximum is exactly 1.5 * 2^(k+2): e is kept", single(3, [7]), 130)
    # 6 + 0.5 * 2^-20 ... cannot be had from one peer; one ulp above comes from a sum: 6 * 2^k + 0.5 * 2^(k-22)
    def ulp_above(xs, es, b):
        single(3, [7])(xs, es, b)
        xs[1][_span(b).start + 5] = 1       # 0.5
        es[1][b] = 127 + 3 + 2 - 22         # times 2^(k - 20): 6 * 2^3 has the ulp 2^(5 - 23), and 0.5 * 2^-17 = 2^-18 is it
    case("one ulp above 1.5 * 2^(k+2): e moves up", ulp_above, 131)
    case("1.5 * 2^k from 1.5: mantissa on the threshold", single(0, [3]), 127 - 2)
    case("4 + 3 = 7 = 1.75 * 2^2: above the threshold, a bump", single(0, [6, 5]), 127 + 2 - 2 + 1)

    def overflow(xs, es, b):
        for x, e in zip(xs, es):
            x[_span(b)] = 7
            e[b] = 254
    case("scale 254 and elements 6: S is inf", overflow, 255, 0)

    def nan_scale(xs, es, b):
        es[1][b] = 255
    case("a peer's scale byte is 255", nan_scale, 255, 0)

    def zero_scale(xs, es, b):
        for x, e in zip(xs, es):
            x[_span(b)] = 1  # 0.5 * 2^-127 = 2^-128 per peer: S = 1.5 * 2^-127, an f32 subnormal; y = 1.5
            e[b] = 0
    case("scale byte 0: 2^-127, S is an f32 subnormal", zero_scale, 0, 3)

    def zeros(xs, es, b):
        for x in xs:
            x[_span(b)] = 0
    case("an all-zero block", zeros, 0, 0)

    base_q, base_e = M.expected("allreduce", *_base(3), "sum", "same")
    for name, (xs, es, want_e, want_q) in cases.items():
        S = M.values("allreduce", xs, es)
        if "ulp" in name:
            assert S[5].view(np.uint32) == np.float32(48).view(np.uint32) + 1, hex(int(S[5].view(np.uint32)))
        got, got_sc = check("allreduce", xs, es, "sum", "same", what=name)
        for b in PLACES:
            assert got_sc[b] == want_e, (name, b, int(got_sc[b]), want_e)
            if want_q is not None:
                assert (got[_span(b)] == want_q).all(), (name, b)
        for b in NEIGHBOURS:  # untouched by the decided block beside them
            assert got_sc[b] == base_e[b] and np.array_equal(got[_span(b)], base_q[_span(b)]), (name, b)
        got32, _ = check("reduce_ltr", xs, es, "sum", "f32", what=name)
        if "255" in name:
            for b in PLACES:
                assert np.isnan(got32[_span(b)]).all(), (name, b)


# ---- 3. quantize / dequantize -----------------------------------------------------------------------------------------
def test_dequantize_every_byte_under_every_scale(device):
    """Every byte (both nibbles) under each of the 256 scale bytes: scale s holds blocks 16 s .. 16 s + 15, whose 256
    bytes are the 256 byte values. To f32; a sample (every 16th scale) to f16 and bf16."""
    raw = np.tile(np.arange(256, dtype=np.uint8), 256)
    e = np.repeat(np.arange(256, dtype=np.uint8), 16)
    n = 2 * raw.size
    codes = M.unpack(raw, n)
    v = M.dequant(codes, e)
    src, sc = bytes_bucket(raw, F4, n=n), bytes_bucket(e, DType.F8E8M0, 1)
    d32 = Bucket(n, DType.F32)
    fmi_amd.mx_dequantize(d32, src, sc)
    fmi_amd.sync()
    M.assert_mx(d32.numpy(), None, v, None, "f32", "every byte x every scale -> f32")
    keep = (np.arange(256) % 16 == 0)
    raw2, e2 = raw[np.repeat(keep, 256)], e[np.repeat(keep, 16)]
    n2 = 2 * raw2.size
    v2 = M.dequant(M.unpack(raw2, n2), e2)
    src2, sc2 = bytes_bucket(raw2, F4, n=n2), bytes_bucket(e2, DType.F8E8M0, 1)
    for kind, dt in (("f16", DType.F16), ("bf16", DType.BF16)):
        d = Bucket(n2, dt)
        fmi_amd.mx_dequantize(d, src2, sc2)
        fmi_amd.sync()
        with np.errstate(all="ignore"):
            H.assert_bits(d.numpy().view(np.uint16), H.narrow(v2, kind), kind, "sum", f"-> {kind}")


def test_fused_widening_of_every_byte_under_every_scale(device):
    """The same table through the FUSED kernel (its hardware widening): P = 2 with a second peer of zeros under scale
    2^0, f32 output: v + 0 is v (and -0 + 0 is +0, NaN stays NaN, as the definition's sum says)."""
    raw = np.tile(np.arange(256, dtype=np.uint8), 256)
    e = np.repeat(np.arange(256, dtype=np.uint8), 16)
    n = 2 * raw.size
    xs = [M.unpack(raw, n), np.zeros(n, np.uint8)]
    es = [e, np.full(e.size, 127, np.uint8)]
    check("allreduce", xs, es, "sum", "f32", what="every byte x every scale")
    check("reduce_ltr", [xs[1], xs[0]], [es[1], es[0]], "sum", "f32", what="every byte x every scale, swapped")


def _scaled_boundaries():
    """The f32 boundary set brought into a few binades: blocks of 32 consecutive boundary values (so a block's maximum
    decides its scale and its other elements land anywhere below), times 2^-100, 1 and 2^100."""
    b = F.boundary_f32()
    b = b[np.isfinite(b)]
    with np.errstate(all="ignore"):
        parts = [(b * np.float32(2.0 ** k)).astype(np.float32) for k in (-100, 0, 100)]
    parts.append(F.boundary_f32()[:4096 * 32])  # with the infs and NaNs of the first blocks left in
    return np.concatenate(parts)


def test_quantize_boundaries_and_every_bf16_pattern(device):
    for name, S, src in (("boundary f32", _scaled_boundaries(), None),
                         ("every bf16 pattern", H.widen(np.arange(65536, dtype=np.uint16), "bf16"), np.arange(65536, dtype=np.uint16))):
        want, want_sc = M.quant(S)
        if src is None:
            b = Bucket.from_numpy(S)
        else:
            b = Bucket(src.size, DType.BF16)
            b.upload(src)
        o = Out(S.size, "same")
        fmi_amd.mx_quantize(o.b, o.sc, b)
        fmi_amd.sync()
        got, got_sc = o.read(name)
        M.assert_mx(got, got_sc, want, want_sc, "same", f"quantize {name}")


def test_fused_narrowing_at_every_tie_and_its_neighbours(device):
    """The FUSED kernel's narrowing (the hardware conversion) cannot be fed arbitrary f32 values: what reaches it is a
    sum of E2M1 values under their scales. So: peer 0 holds code a at 2^0, peer 1 code b at 2^-1 (a + b / 2 covers every
    magnitude and every one of the seven ties, both signs), peer 2 nothing, or +-0.5 at 2^-20 .. 2^-25 (the tie's f32
    neighbours and values just off it). One combination per block at element 0; element 1 is 6, which keeps the block's
    scale at 2^0 wherever |a + b / 2| <= 6, so that y is the sum itself."""
    a, b, c = np.meshgrid(np.arange(16), np.arange(16), np.arange(13), indexing="ij")
    a, b, c = a.ravel().astype(np.uint8), b.ravel().astype(np.uint8), c.ravel()
    nb = a.size
    xs = [np.zeros(32 * nb, np.uint8) for _ in range(3)]
    xs[0][0::32], xs[1][0::32] = a, b
    xs[2][0::32] = np.where(c == 0, 0, np.where(c % 2 == 1, 1, 9))  # 0, +0.5, -0.5
    xs[0][1::32] = 7
    es = [np.full(nb, 127, np.uint8), np.full(nb, 126, np.uint8), (127 - 20 - (np.maximum(c, 1) - 1) // 2).astype(np.uint8)]
    S = M.values("allreduce", xs, es)
    y, ee, _ = M.scaled(S)
    for v, _code in M.TIES:  # the ties and both f32 neighbours of each are among what the narrowing is fed
        for w in (v, -v):
            w = np.float32(w)
            for t in (w, np.nextafter(w, np.float32(0)), np.nextafter(w, np.float32(8) * np.sign(w))):
                assert (y[0::32] == t).any(), float(t)
    check("allreduce", xs, es, "sum", "same", what="ties and neighbours")


@pytest.mark.parametrize("offset", [1, 3])
def test_quantize_dequantize_unaligned_odd_and_empty(device, offset):
    n = N_TILE  # odd
    xs, es = cut(*inputs(1, (120, 134)), n)
    q, e = fp4_bucket(xs[0], offset), bytes_bucket(es[0], DType.F8E8M0, offset)
    whole = Bucket(n + offset, DType.F32)
    wide = whole.view(offset, n)  # 4 and 12 bytes off 16-B alignment
    fmi_amd.mx_dequantize(wide, q, e)
    o = Out(n, "same", offset)
    fmi_amd.mx_quantize(o.b, o.sc, wide)
    fmi_amd.sync()
    v = M.dequant(xs[0], es[0])
    M.assert_mx(wide.numpy(), None, v, None, "f32", "unaligned dequantize")
    want, want_sc = M.quant(v)
    got, got_sc = o.read("unaligned quantize")  # checks the guard bytes and the last high nibble
    M.assert_mx(got, got_sc, want, want_sc, "same", "unaligned quantize")
    # n = 0 succeeds and writes nothing
    lib = fmi_amd.load()
    assert lib.fmi_dev_mx_quantize(int(F4), o.b.ptr, o.sc.ptr, int(DType.F32), wide.ptr, 0, None) == 0
    assert lib.fmi_dev_mx_dequantize(int(DType.F32), wide.ptr, int(F4), q.ptr, e.ptr, 0, None) == 0
    ins, scs = (ctypes.c_void_p * 1)(q.ptr), (ctypes.c_void_p * 1)(e.ptr)
    assert lib.fmi_dev_reduce_tree_mx(0, int(F4), 0, int(F4), o.b.ptr, o.sc.ptr, ins, scs, 1, 0, 0, None) == 0
    fmi_amd.sync()
    again, again_sc = o.read("after the empty calls")
    assert np.array_equal(again, got) and np.array_equal(again_sc, got_sc)


# ---- 4. beyond the fused kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["same", "f32"])
@pytest.mark.parametrize("P", [1, 17, 33])
def test_fallback_peer_counts(device, P, out):
    """P = 1 (not a copy: it requantizes), 17 and 33 (f32 temporaries): the definition's bits."""
    xs, es = cut(*inputs(P), N_TILE)
    for name in ALGS:
        check(name, xs, es, "sum", out, what="fallback")
    check("allreduce", xs, es, "avg", out, what="fallback")
    check("allreduce", *cut(xs, es, 31), "sum", out, what="fallback")


@pytest.mark.parametrize("out", ["same", "f32"])
def test_fallback_unaligned(device, out):
    xs, es = cut(*inputs(3), N_TILE)
    for name in ALGS:
        check(name, xs, es, "sum", out, offset=1, what="1-byte offset")
    check("reduce_ltr", xs, es, "avg", out, offset=3, what="3-byte offset")


# ---- 5. in place ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, -1])
def test_in_place(device, which):
    """out / out_scales are ins[p] / in_scales[p] themselves, p the first or the last peer."""
    P = 8
    xs, es = cut(*inputs(P), N_TILE)
    for name in ALGS:
        family, alg, root_of = ALGS[name]
        ins, scs = [fp4_bucket(x) for x in xs], [bytes_bucket(e, DType.F8E8M0, 1) for e in es]
        fmi_amd.reduce_tree_mx(Op.SUM, alg, ins[which], scs[which], ins, scs, rank=root_of(P))
        fmi_amd.sync()
        want, want_sc = M.expected(family, xs, es, "sum", "same", root_of(P))
        M.assert_mx(M.unpack(ins[which].numpy(), N_TILE), scs[which].numpy(), want, want_sc, "same", f"in place {name} peer {which}")
        for p in range(1, P - 1):
            assert np.array_equal(ins[p].numpy(), M.pack(xs[p])) and np.array_equal(scs[p].numpy(), es[p])


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------
def test_graph_replay_reads_new_elements_and_scales(device):
    P, n = 8, N_FUSED
    old, new = inputs(P), inputs(P, seed=8)
    ins, scs = [fp4_bucket(x) for x in old[0]], [bytes_bucket(e, DType.F8E8M0, 1) for e in old[1]]
    o = Out(n, "same")
    fmi_amd.sync()
    st = Stream()
    g = Graph.capture(st, lambda: fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, o.b, o.sc, ins, scs, stream=st))
    try:
        for xs, es in (old, new):
            for b, x in zip(ins, xs):
                b.upload(M.pack(x))
            for b, e in zip(scs, es):
                b.upload(e)
            g.launch(st)
            st.sync()
            want, want_sc = M.expected("allreduce", xs, es)
            got, got_sc = o.read("graph replay")
            M.assert_mx(got, got_sc, want, want_sc, "same", "graph replay")
    finally:
        g.destroy()
        st.destroy()


# ---- 7. the communicator: LOCAL transport, every rank compared ---------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("N", [2, 3, 8])
def test_comm_allreduce_mx(device, N, ragged):
    from tests.test_gpu_comm import run_ranks

    n = 64 * N * 3 + (45 if ragged else 0)  # ragged AND odd
    xs, es = M.random_inputs(n, N, 81, 112, 142)

    def body(c, r):
        send, ssc, res = fp4_bucket(xs[r]), bytes_bucket(es[r], DType.F8E8M0, 1), {}
        for out in ("same", "f32"):
            for op, ordered in (("sum", False), ("sum", True), ("avg", False)):
                o = Out(n, out)
                c.allreduce_mx(OP[op], send, ssc, o.b, o.sc, ordered=ordered)
                fmi_amd.sync()
                res[out, op, ordered] = o.read(f"rank {r}")
        res["send"] = (send.numpy(), ssc.numpy())
        return res

    res = run_ranks(N, body)
    for out in ("same", "f32"):
        for op, ordered in (("sum", False), ("sum", True), ("avg", False)):
            want, want_sc = M.expected("allreduce_ltr" if ordered else "allreduce", xs, es, op, out)
            for r in range(N):
                got, got_sc = res[r][out, op, ordered]
                M.assert_mx(got, got_sc, want, want_sc, out, f"N={N} n={n} out={out} {op} ordered={ordered} rank {r}")
    for r in range(N):
        assert np.array_equal(res[r]["send"][0], M.pack(xs[r])) and np.array_equal(res[r]["send"][1], es[r]), f"send of rank {r} was modified"


def test_one_rank_communicator_runs_the_p1_form(device):
    from tests.test_gpu_comm import run_ranks

    n = 1001
    xs, es = M.random_inputs(n, 1, 85)
    xs = [xs[0] & 0xB]  # magnitudes up to 1.5: every block has headroom, so its canonical scale byte is two below its own

    def body(c, r):
        o = Out(n, "same")
        c.allreduce_mx(Op.SUM, fp4_bucket(xs[0]), bytes_bucket(es[0], DType.F8E8M0, 1), o.b, o.sc)
        fmi_amd.sync()
        return o.read("one rank")

    got, got_sc = run_ranks(1, body)[0]
    want, want_sc = M.expected("allreduce", xs, es)
    M.assert_mx(got, got_sc, want, want_sc, "same", "one rank")
    assert (got_sc < es[0]).all(), "P = 1 requantizes: blocks with headroom do not keep their scale bytes"


# ---- 8. the upper layers ---------------------------------------------------------------------------------------------------
def test_bucket_round_trips_packed_bytes(device):
    codes = inputs(1)[0][0][:77]
    b = Bucket(77, F4)
    assert b.nbytes == 39
    b.upload(fmi_amd.fp4_pack(codes))
    assert np.array_equal(fmi_amd.fp4_unpack(b.numpy(), 77), codes)
    g = Bucket.group(3, 77, F4)
    assert all(x.nbytes == 39 for x in g)
    g[0].copy_from(b)
    fmi_amd.sync()
    assert np.array_equal(g[0].numpy(), b.numpy())
    with pytest.raises(ValueError, match="F4E2M1"):
        fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, g[0], g[1:])


def test_torch_glue(device):
    """HipEngine.reduce_tree_mx on torch.float4_e2m1fn_x2 device tensors with float8_e8m0fnu scale tensors (a child
    process: torch must be loaded before the library) equals the definition."""
    r = subprocess.run([sys.executable, "-u", "-m", "tests._mxfp4_torch_worker"], cwd=ROOT, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0 and "mxfp4 torch glue ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
