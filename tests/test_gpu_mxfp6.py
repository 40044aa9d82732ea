"""MXFP6 on the GPU (FMI_F6E2M3 / FMI_F6E3M2 in fmi_dev_reduce_tree_mx, fmi_dev_mx_quantize, fmi_dev_mx_dequantize,
fmi_comm_allreduce_mx and their stochastic-rounding forms), bit for bit against tests/_mxfp6.py: the packed bytes and the
scale bytes exactly, an f32 output on its uint32 view (a NaN matching any NaN).

Containment: every output lies in guarded, poisoned bytes (tests/_guard.py; the FP6 Bucket is laid over a guarded
allocation made at DType.U8, so exactly ceil(3 n / 4) bytes and ceil(n / 32) scale bytes may change and every one of them
must), the poison is proven absent from the expected bytes on the CPU (two poisons where every candidate occurs), and
the inputs are frozen. The packed bytes are compared whole, so the last byte's spare bits are 0. Scale arrays sit at
odd addresses."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fmi_amd
from fmi_amd import Alg, Bucket, DType, Graph, Op, Stream, Tune
from tests import _guard as G
from tests import _half as H
from tests import _mx as MX
from tests import _mx_sr as SR
from tests import _mxfp6 as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"e2m3": DType.F6E2M3, "e3m2": DType.F6E3M2}
OP = {"sum": Op.SUM, "avg": Op.AVG}
KINDS = M.KINDS
TILE = M.TILE                                        # 16,384 elements: two blocks per lane, 256 lanes
BIG = tuple(TILE + 96 + r for r in (17, 18, 19, 20))  # an odd count of extra whole blocks and every n % 4
SMALL = (1, 3, 31, 32, 33, 63, 64, 65)
N_LONG = BIG[-1]
PEERS = (2, 3, 8, 13, 16)
ALGS = {
    "allreduce": ("allreduce", Alg.ALLREDUCE),
    "reduce": ("reduce", Alg.REDUCE),
    "reduce_ltr": ("reduce_ltr", Alg.REDUCE_LTR),
}


@functools.lru_cache(maxsize=None)
def inputs(P, rng=M.ORDER_RANGE, n=N_LONG, seed=None):
    """The default is M.order_inputs(P, n): cut() of it to 8305 or 12295 is the data tests/test_mxfp6_cpu.py asserts the
    bracketings to differ on, because a shorter bucket is a prefix of a longer one. Shared and never modified."""
    xs, es = M.random_inputs(n, P, 1000 + P if seed is None else seed, *rng)
    for a in xs + es:
        a.setflags(write=False)
    return tuple(xs), tuple(es)


def cut(xs, es, n):
    return [x[:n] for x in xs], [e[:MX.blocks(n)] for e in es]


def over(b, n, dtype):
    """The bucket of n elements of `dtype` laid over the guarded U8 body b."""
    return Bucket(n, dtype, ptr=b.ptr, owner=b)


class Frozen:
    """FP6 inputs and their scale bytes in guarded regions. offset: bytes off 16-B alignment (elements); scales 1 byte off."""

    def __init__(self, kind, xs, es, offset=0):
        n = len(xs[0])
        self.el = G.frozen([M.pack(x) for x in xs], DType.U8, offset)
        self.sc = G.frozen(list(es), DType.U8, 1)
        self.ins = [over(b, n, DT[kind]) for b in self.el.bs]
        self.scs = [over(b, MX.blocks(n), DType.F8E8M0) for b in self.sc.bs]

    def assert_intact(self, what):
        self.el.assert_intact(what + " elements")
        self.sc.assert_intact(what + " scales")


def outputs(kind, want, want_sc, n, offset=0):
    """Guarded element and scale outputs, one pair per poison that the case needs: (element Guarded, scale Guarded,
    FP6 bucket, scale bucket)."""
    ge = G.guarded_runs(M.pack(want), M.nbytes(n), DType.U8, offset)
    gs = G.guarded_runs(want_sc, MX.blocks(n), DType.U8, 1)
    for k in range(max(len(ge), len(gs))):
        a, b = ge[k % len(ge)], gs[k % len(gs)]
        if k >= len(ge):
            a.repoison()
        if k >= len(gs):
            b.repoison()
        yield a, b, over(a.b, n, DT[kind]), over(b.b, MX.blocks(n), DType.F8E8M0)


def judge(kind, a, b, want, want_sc, n, what):
    raw = a.read(M.pack(want), what)
    got_sc = b.read(want_sc, what + " scales")
    M.assert_mx(M.unpack(raw, n), got_sc, want, want_sc, "same", what)
    assert np.array_equal(raw, M.pack(want)), f"{what}: the last byte's spare bits are not 0"


def check(kind, name, xs, es, op="sum", out="same", root=0, offset=0, seed=None, first=0, what=""):
    family, alg = ALGS[name]
    P, n = len(xs), len(xs[0])
    what = f"{what} {kind} {name} {op} P={P} n={n} out={out} root={root} offset={offset}"
    fr = Frozen(kind, xs, es, offset)
    if out == "f32":
        want = M.values(family, kind, xs, es, op, root)
        for got in G.launched(want, n, DType.F32, lambda o: fmi_amd.reduce_tree_mx(OP[op], alg, o, None, fr.ins, fr.scs, rank=root), what, offset):
            M.assert_mx(got, None, want, None, "f32", what)
    else:
        want, want_sc = M.expected(family, kind, xs, es, op, "same", root) if seed is None else M.expected_sr(family, kind, xs, es, seed, first, op, root)
        word = None if seed is None else G.frozen([np.array([seed], np.uint64)], DType.U64)
        for a, b, o, osc in outputs(kind, want, want_sc, n, offset):
            fmi_amd.reduce_tree_mx(OP[op], alg, o, osc, fr.ins, fr.scs, rank=root, seed=None if word is None else word.bs[0], first=first)
            fmi_amd.sync()
            judge(kind, a, b, want, want_sc, n, what)
        if word is not None:
            word.assert_intact(what + " seed")
    fr.assert_intact(what)


# ---- 1. the fused kernels -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["same", "f32"])
@pytest.mark.parametrize("P", PEERS)
@pytest.mark.parametrize("kind", KINDS)
def test_fused_every_algorithm_and_root(device, kind, P, out):
    """One big size and one small one at every algorithm and every root / rank; SUM everywhere, the mean at rank 0."""
    xs, es = inputs(P)
    for n in (BIG[0], 33):
        cx, ce = cut(xs, es, n)
        for name in ALGS:
            roots = range(P) if n == 33 or P <= 3 else (0, P - 1)
            for root in roots:
                check(kind, name, cx, ce, "sum", out, root)
        check(kind, "allreduce", cx, ce, "avg", out)
        check(kind, "reduce", cx, ce, "avg", out, P - 1)


@pytest.mark.parametrize("out", ["same", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_every_size(device, kind, out):
    xs, es = inputs(8)
    for n in SMALL + BIG:
        check(kind, "allreduce", *cut(xs, es, n), "sum", out)
        check(kind, "reduce_ltr", *cut(xs, es, n), "avg", out)
    xs, es = inputs(3, M.EXACT_RANGE)
    for n in BIG:
        check(kind, "reduce", *cut(xs, es, n), "sum", out, 2)


@pytest.mark.parametrize("policy", [0, 2])
def test_fused_both_access_policies(device, policy):
    before = fmi_amd.tune_get(Tune.FUSED_POLICY)
    fmi_amd.tune_set(Tune.FUSED_POLICY, policy)
    try:
        for kind in KINDS:
            for P in (3, 8):
                xs, es = inputs(P)
                for n in (BIG[1], BIG[2]):
                    for out in ("same", "f32"):
                        check(kind, "allreduce", *cut(xs, es, n), "sum", out, what=f"policy {policy}")
            check(kind, "allreduce", *cut(*inputs(8), BIG[0]), "sum", "same", seed=SR.SEEDS[2], first=32, what=f"policy {policy} sr")
    finally:
        fmi_amd.tune_set(Tune.FUSED_POLICY, before)


@pytest.mark.parametrize("P", M.ORDER_PEERS)
@pytest.mark.parametrize("kind", KINDS)
def test_order(device, kind, P):
    """The order cases of tests/test_mxfp6_cpu.py: f32 output, scale bytes 112..142, REDUCE at root P - 1."""
    xs, es = inputs(P)
    for n in M.ORDER_SIZES:
        for name, root in (("allreduce", 0), ("reduce", P - 1), ("reduce_ltr", 0)):
            check(kind, name, *cut(xs, es, n), "sum", "f32", root, what="order")


# ---- 2. the fallback route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["same", "f32"])
@pytest.mark.parametrize("P", [1, 17])
@pytest.mark.parametrize("kind", KINDS)
def test_fallback_peer_counts(device, kind, P, out):
    xs, es = inputs(P)
    for n in (BIG[0], BIG[3], 31):
        for name in ALGS:
            check(kind, name, *cut(xs, es, n), "sum", out, what="fallback")
    check(kind, "allreduce", *cut(xs, es, BIG[1]), "avg", out, what="fallback")


@pytest.mark.parametrize("out", ["same", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_fallback_unaligned(device, kind, out):
    xs, es = inputs(3)
    for n in SMALL + BIG:
        check(kind, "allreduce", *cut(xs, es, n), "sum", out, offset=1, what="1 byte off")
    check(kind, "reduce_ltr", *cut(xs, es, BIG[2]), "avg", out, offset=1, what="1 byte off")


# ---- 3. in place, graph capture ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, -1])
@pytest.mark.parametrize("kind", KINDS)
def test_in_place(device, kind, which):
    P = 8
    for n in (BIG[0], BIG[3]):
        xs, es = cut(*inputs(P), n)
        for name, (family, alg) in ALGS.items():
            root = P - 1 if name == "reduce" else 0
            el = G.Guarded(M.nbytes(n), DType.U8, count=P).load([M.pack(x) for x in xs])
            sc = G.Guarded(MX.blocks(n), DType.U8, 1, count=P).load(list(es))
            ins, scs = [over(b, n, DT[kind]) for b in el.bs], [over(b, MX.blocks(n), DType.F8E8M0) for b in sc.bs]
            fmi_amd.reduce_tree_mx(Op.SUM, alg, ins[which], scs[which], ins, scs, rank=root)
            fmi_amd.sync()
            want, want_sc = M.expected(family, kind, xs, es, "sum", "same", root)
            got, got_sc = el.read_all([None] * P, "in place"), sc.read_all([None] * P, "in place scales")
            w = which % P
            assert np.array_equal(got[w], M.pack(want)) and np.array_equal(got_sc[w], want_sc), f"in place {kind} {name} peer {which} n={n}"
            for p in range(P):
                if p != w:
                    assert np.array_equal(got[p], M.pack(xs[p])) and np.array_equal(got_sc[p], es[p]), f"peer {p} was modified"


@pytest.mark.parametrize("kind", KINDS)
def test_graph_replays_with_new_inputs_and_a_new_seed(device, kind):
    P, n = 8, BIG[2]
    old, new = cut(*inputs(P), n), cut(*inputs(P, seed=8), n)
    ins = [over(Bucket.from_numpy(M.pack(x)), n, DT[kind]) for x in old[0]]
    scs = [Bucket(MX.blocks(n), DType.F8E8M0) for _ in old[1]]
    word = Bucket.from_numpy(np.array([SR.SEEDS[1]], np.uint64))
    want0, want0_sc = M.expected("allreduce", kind, *old)
    (a, b, o, osc), = list(outputs(kind, want0, want0_sc, n))[:1]
    (a2, b2, o2, osc2), = list(outputs(kind, want0, want0_sc, n))[:1]
    fmi_amd.sync()
    st = Stream()

    def both():
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, o, osc, ins, scs, stream=st)
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, o2, osc2, ins, scs, stream=st, seed=word, first=64)

    g = Graph.capture(st, both)
    try:
        for (xs, es), seed in ((old, SR.SEEDS[1]), (new, SR.SEEDS[2])):
            for bkt, x in zip(ins, xs):
                bkt.upload(M.pack(x))
            for bkt, e in zip(scs, es):
                bkt.upload(e)
            word.upload(np.array([seed], np.uint64))
            for r in (a, b, a2, b2):
                r.repoison()
            g.launch(st)
            st.sync()
            want, want_sc = M.expected("allreduce", kind, xs, es)
            raw, got_sc = a.read(None, "graph"), b.read(None, "graph scales")
            assert np.array_equal(raw, M.pack(want)) and np.array_equal(got_sc, want_sc), "graph replay"
            want, want_sc = M.expected_sr("allreduce", kind, xs, es, seed, 64)
            raw, got_sc = a2.read(None, "graph sr"), b2.read(None, "graph sr scales")
            assert np.array_equal(raw, M.pack(want)) and np.array_equal(got_sc, want_sc), "graph replay, stochastic rounding"
    finally:
        g.destroy()
        st.destroy()


# ---- 4. widen and narrow, exhaustively ------------------------------------------------------------------------------
def _every_code_everywhere():
    """Block (s, t), s a scale byte and t = 0..63, holds code (i + t) % 64 at position i: all 64 codes at every one of
    the 32 positions under all 256 scale bytes. 524,288 elements."""
    t = np.arange(64)[:, None]
    i = np.arange(32)[None, :]
    one = ((i + t) % 64).astype(np.uint8).ravel()
    return np.tile(one, 256), np.repeat(np.arange(256, dtype=np.uint8), 64)


@pytest.mark.parametrize("kind", KINDS)
def test_widen_every_code_at_every_position_under_every_scale(device, kind):
    codes, e = _every_code_everywhere()
    n = codes.size
    v = M.dequant(codes, e, kind)
    fr = Frozen(kind, [codes], [e])
    for got in G.launched(v, n, DType.F32, lambda o: fmi_amd.mx_dequantize(o, fr.ins[0], fr.scs[0]), "dequantize"):
        M.assert_mx(got, None, v, None, "f32", f"{kind} dequantize: every code x position x scale")
    # a sample (every 16th scale byte) to f16 and bf16
    keep = np.repeat(np.arange(256) % 16 == 0, 64)
    c2, e2 = codes[np.repeat(keep, 32)], e[keep]
    v2 = M.dequant(c2, e2, kind)
    fr2 = Frozen(kind, [c2], [e2])
    for k, dt in (("f16", DType.F16), ("bf16", DType.BF16)):
        d = Bucket(c2.size, dt)
        fmi_amd.mx_dequantize(d, fr2.ins[0], fr2.scs[0])
        fmi_amd.sync()
        with np.errstate(all="ignore"):
            H.assert_bits(d.numpy().view(np.uint16), H.narrow(v2, k), k, "sum", f"{kind} -> {k}")
    # the FUSED kernel (its hardware widening): P = 2, the second peer all +0 under scale byte 127, f32 output
    xs, es = [codes, np.zeros(n, np.uint8)], [e, np.full(e.size, 127, np.uint8)]
    check(kind, "allreduce", xs, es, "sum", "f32", what="every code x position x scale")
    check(kind, "reduce_ltr", xs[::-1], es[::-1], "sum", "f32", what="every code x position x scale, swapped")


@pytest.mark.parametrize("kind", KINDS)
def test_narrow_every_grid_value_tie_and_neighbour(device, kind):
    vals = M.exhaustive_values(kind)
    for t, _ in M.ties(kind):
        for w in (t, -t):
            for x in (w, np.nextafter(np.float32(w), np.float32(0)), np.nextafter(np.float32(w), np.float32(64 * np.sign(w)))):
                assert (vals == np.float32(x)).any(), float(x)
    S = M.pinned_blocks(np.tile(vals, 2)[:vals.size + 17], kind)  # shifted once, so a value meets other positions
    want, want_sc = M.quant(S, kind)
    assert (want_sc == 127).all()
    src = G.frozen([S], DType.F32)
    for a, b, o, osc in outputs(kind, want, want_sc, S.size):
        fmi_amd.mx_quantize(o, osc, src.bs[0])
        fmi_amd.sync()
        judge(kind, a, b, want, want_sc, S.size, f"{kind} quantize: ties and neighbours")
    src.assert_intact("quantize")


def _pow2(x):
    return x > 0 and np.frexp(x)[0] == 0.5


@pytest.mark.parametrize("kind", KINDS)
def test_fused_narrowing_at_every_tie_and_its_neighbours(device, kind):
    """The fused kernel's narrowing is fed sums of elements under their scales, so a target y = hi + t2 + t3: peer 0 holds
    the grid value below |y| at 2^0, peers 1 and 2 the code of 1.0 under the scale bytes of the two powers of two that
    make up the rest (the half step of a tie, and one f32 ulp up or down). One target per block at element 1, every
    position of a lane pair in turn; element 0 is the largest value, so e_out = 127 and the inverse scale is 1. Targets
    whose rest is no such sum are left to the quantize test above."""
    Gd = M.MAGNITUDES[kind].astype(np.float64)
    one = int(np.flatnonzero(Gd == 1.0)[0])
    rows = []
    for y in M.exhaustive_values(kind).astype(np.float64):
        a = abs(y)
        lo = int(np.searchsorted(Gd, a, side="right") - 1)
        rem = a - Gd[lo]
        if rem == 0:
            parts = (0.0, 0.0)
        elif _pow2(rem):
            parts = (rem, 0.0)
        else:
            t = 2.0 ** np.floor(np.log2(rem))
            parts = (t, rem - t) if _pow2(rem - t) else (2 * t, rem - 2 * t) if _pow2(2 * t - rem) else None
        if parts is not None and all(t == 0 or abs(t) >= 2.0 ** -100 for t in parts):  # the f32 neighbours of 0 have no scale byte
            rows.append((y, lo, parts))
    nb = len(rows)
    xs = [np.zeros(32 * nb, np.uint8) for _ in range(3)]
    es = [np.full(nb, 127, np.uint8) for _ in range(3)]
    want_y = np.zeros(nb, np.float32)
    for k, (y, lo, parts) in enumerate(rows):
        neg = 0x20 if np.signbit(y) else 0
        pos = 1 + k % 31
        xs[0][32 * k] = 31
        xs[0][32 * k + pos] = lo | neg
        for p, t in ((1, parts[0]), (2, parts[1])):
            xs[p][32 * k + pos] = neg  # a zero of y's sign: -0 + -0 is -0
            if t != 0:
                xs[p][32 * k + pos] = one | (neg if t > 0 else 0x20 - neg)
                es[p][k] = 127 + int(np.log2(abs(t)))
        want_y[k] = y
    S = M.values("allreduce", kind, xs, es)
    got_y = S.reshape(nb, 32)[np.arange(nb), 1 + np.arange(nb) % 31]
    assert np.array_equal(got_y.view(np.uint32), want_y.view(np.uint32)), "the construction does not give its targets"
    for t, _ in M.ties(kind):
        for w in (t, -t):
            for x in (w, np.nextafter(np.float32(w), np.float32(0)), np.nextafter(np.float32(w), np.float32(64 * np.sign(w)))):
                assert (want_y == np.float32(x)).any(), float(x)
    assert (M.scale_bytes(S, kind) == 127).all()
    check(kind, "allreduce", xs, es, "sum", "same", what="ties and neighbours")


@pytest.mark.parametrize("kind", KINDS)
def test_quantize_every_bf16_pattern_within_range(device, kind):
    pat = np.arange(65536, dtype=np.uint16)
    w = H.widen(pat, "bf16")
    pat = pat[np.abs(w) <= M.MAX[kind]]  # drops the NaNs too
    S = H.widen(pat, "bf16")
    want, want_sc = M.quant(S, kind)
    src = G.frozen([pat], DType.BF16)
    for a, b, o, osc in outputs(kind, want, want_sc, S.size):
        fmi_amd.mx_quantize(o, osc, src.bs[0])
        fmi_amd.sync()
        judge(kind, a, b, want, want_sc, S.size, f"{kind} quantize of every bf16 pattern")
    src.assert_intact("quantize bf16")


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_quantize_dequantize_every_size(device, kind, offset):
    xs, es = inputs(1, M.EXACT_RANGE)
    for n in SMALL + BIG:
        cx, ce = cut(xs, es, n)
        v = M.dequant(cx[0], ce[0], kind)
        fr = Frozen(kind, cx, ce, offset)
        for got in G.launched(v, n, DType.F32, lambda o: fmi_amd.mx_dequantize(o, fr.ins[0], fr.scs[0]), "dequantize", offset):
            M.assert_mx(got, None, v, None, "f32", f"{kind} dequantize n={n} offset={offset}")
        want, want_sc = M.quant(v, kind)
        src = G.frozen([v], DType.F32, offset)
        for a, b, o, osc in outputs(kind, want, want_sc, n, offset):
            fmi_amd.mx_quantize(o, osc, src.bs[0])
            fmi_amd.sync()
            judge(kind, a, b, want, want_sc, n, f"{kind} quantize n={n} offset={offset}")
        fr.assert_intact("dequantize")


# ---- 5. stochastic rounding -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_sr_seeds_and_firsts(device, kind):
    """Fused (aligned) and fallback (one byte off) both equal the definition, and so each other."""
    P = 8
    xs, es = M.visible_inputs(kind, BIG[1], P)
    rne = M.expected("allreduce", kind, xs, es)
    for seed in SR.SEEDS:
        for first in SR.FIRSTS:
            check(kind, "allreduce", xs, es, "sum", "same", seed=seed, first=first, what="sr")
            sr = M.expected_sr("allreduce", kind, xs, es, seed, first)
            assert np.array_equal(sr[1], rne[1]), "the scale bytes are the round-to-nearest call's"
    assert (M.expected_sr("allreduce", kind, xs, es, 1)[0] != rne[0]).mean() > 0.05, "the inputs do not show the rounding"
    for n in SMALL + BIG[2:]:
        check(kind, "reduce_ltr", *cut(xs, es, n), "avg", "same", seed=SR.SEEDS[2], first=SR.FIRSTS[2], what="sr sizes")
    check(kind, "allreduce", xs, es, "sum", "same", offset=1, seed=SR.SEEDS[2], first=32, what="sr fallback")
    check(kind, "reduce", *cut(*M.visible_inputs(kind, BIG[0], 17), BIG[0]), "sum", "same", 16, seed=SR.SEEDS[3], first=32, what="sr P=17")
    check(kind, "allreduce", *M.visible_inputs(kind, BIG[3], 1), "sum", "same", seed=SR.SEEDS[1], first=0, what="sr P=1")


@pytest.mark.parametrize("kind", KINDS)
def test_sr_grid_values_never_move_and_splits_agree(device, kind):
    seed = SR.SEEDS[2]
    word = G.frozen([np.array([seed], np.uint64)], DType.U64)
    # every code under scale 127 from one peer and zeros from the other: y is a grid value (or the block is rescaled by a
    # power of two, which keeps it one)
    codes = np.tile(np.arange(64, dtype=np.uint8), 40)
    n = codes.size
    xs, es = [codes, np.zeros(n, np.uint8)], [np.full(MX.blocks(n), 127, np.uint8)] * 2
    want, want_sc = M.expected("allreduce", kind, xs, es)
    assert np.array_equal(M.expected_sr("allreduce", kind, xs, es, seed, 96)[0], want)
    check(kind, "allreduce", xs, es, "sum", "same", seed=seed, first=96, what="grid values")
    # the quantize call on f32 ties and neighbours, whole and split at a multiple of 32
    S = M.pinned_blocks(np.tile(M.exhaustive_values(kind), 3), kind)
    n, cutat = S.size, 32 * 7
    want, want_sc = M.quant_sr(S, kind, seed, 64)
    src = G.frozen([S], DType.F32)
    for a, b, o, osc in outputs(kind, want, want_sc, n):
        fmi_amd.mx_quantize(o, osc, src.bs[0], seed=word.bs[0], first=64)
        fmi_amd.sync()
        judge(kind, a, b, want, want_sc, n, "quantize sr")
        a.repoison(), b.repoison()
        fmi_amd.mx_quantize(o.view(0, cutat), osc.view(0, cutat // 32), src.bs[0].view(0, cutat), seed=word.bs[0], first=64)
        fmi_amd.mx_quantize(o.view(cutat, n - cutat), osc.view(cutat // 32, MX.blocks(n) - cutat // 32), src.bs[0].view(cutat, n - cutat),
                            seed=word.bs[0], first=64 + cutat)
        fmi_amd.sync()
        judge(kind, a, b, want, want_sc, n, "quantize sr, split")
    host, host_sc = fmi_amd.mx_quantize_sr_host(DT[kind], S, seed, 64)
    assert np.array_equal(host, M.pack(want)) and np.array_equal(host_sc, want_sc)
    word.assert_intact("seed")


# ---- 6. the communicator: LOCAL transport, ranks as threads ----------------------------------------------------------
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_comm_allreduce_mx(device, kind, N):
    from tests.test_gpu_comm import run_ranks

    seed, first = SR.SEEDS[2], 64
    for n in (64 * N * 3, 64 * N * 3 + 45, 64 * N * 2 + 18):  # whole shards; a ragged last shard, n % 4 = 1 and 2
        xs, es = M.random_inputs(n, N, 81, 112, 142)
        wants = {}
        for op, ordered in (("sum", False), ("sum", True), ("avg", False)):
            fam = "allreduce_ltr" if ordered else "allreduce"
            wants["f32", op, ordered] = (M.values(fam, kind, xs, es, op), None)
            wants["same", op, ordered] = M.expected(fam, kind, xs, es, op)
        wants["sr", "sum", False] = M.expected_sr("allreduce", kind, xs, es, seed, first)

        def body(c, r):
            fr = Frozen(kind, [xs[r]], [es[r]])
            word = G.frozen([np.array([seed], np.uint64)], DType.U64)
            for (out, op, ordered), (want, want_sc) in wants.items():
                what = f"{kind} N={N} n={n} {out} {op} ordered={ordered} rank {r}"
                if out == "f32":
                    for got in G.launched(want, n, DType.F32, lambda o: c.allreduce_mx(OP[op], fr.ins[0], fr.scs[0], o, None, ordered=ordered), what):
                        M.assert_mx(got, None, want, None, "f32", what)
                    continue
                for a, b, o, osc in outputs(kind, want, want_sc, n):
                    if out == "sr":
                        c.allreduce_mx(OP[op], fr.ins[0], fr.scs[0], o, osc, seed=word.bs[0], first=first)
                    else:
                        c.allreduce_mx(OP[op], fr.ins[0], fr.scs[0], o, osc, ordered=ordered)
                    fmi_amd.sync()
                    judge(kind, a, b, want, want_sc, n, what)
            fr.assert_intact(f"send of rank {r}")
            return True

        assert all(run_ranks(N, body))


# ---- 7. the upper layers ----------------------------------------------------------------------------------------------
def test_bucket_round_trips_packed_bytes(device):
    codes = inputs(1)[0][0][:77]
    for dt in DT.values():
        b = Bucket(77, dt)
        assert b.nbytes == 58
        b.upload(fmi_amd.fp6_pack(codes))
        assert np.array_equal(fmi_amd.fp6_unpack(b.numpy(), 77), codes)
        g = Bucket.group(3, 77, dt)
        assert all(x.nbytes == 58 for x in g)
        g[0].copy_from(b)
        fmi_amd.sync()
        assert np.array_equal(g[0].numpy(), b.numpy())
        with pytest.raises(ValueError, match=dt.name):
            fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, g[0], g[1:])


def test_torch_glue(device):
    """HipEngine.reduce_tree_mx on packed torch.uint8 device tensors with dtype= and n= (a child process: torch must be
    loaded before the library) equals the definition."""
    r = subprocess.run([sys.executable, "-u", "-m", "tests._mxfp6_torch_worker"], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "mxfp6 torch glue ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
