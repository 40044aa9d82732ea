"""The MX (block-scaled FP8) calls on the GPU (fmi_dev_reduce_tree_mx, fmi_dev_mx_quantize, fmi_dev_mx_dequantize,
fmi_comm_allreduce_mx), bit for bit against tests/_mx.py: element bytes with F.assert_bits and an f32 output on its
uint32 view (a NaN matching any NaN), scale bytes exactly."""
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
from tests.test_gpu_fp8_scaled import N_FUSED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"e4m3": DType.F8E4M3, "e5m2": DType.F8E5M2}
OP = {"sum": Op.SUM, "avg": Op.AVG}
# 4096 + 96 + 17: 131 whole blocks = 262 lane groups (more than one 256-thread tile), 263 lane groups of 16 in all (odd),
# and a ragged block of 17 elements
N_TILE = 4096 + 96 + 17
SIZES = (1, 31, 32, 33, 48, 63, 64, N_TILE, N_FUSED)
THREE_SIZES = (33, N_TILE, N_FUSED)
# (name, oracle family, Alg, root as a function of P)
ALGS = {
    "allreduce": ("allreduce", Alg.ALLREDUCE, lambda P: 0),
    "reduce_rootlast": ("reduce", Alg.REDUCE, lambda P: P - 1),
    "reduce_ltr": ("reduce_ltr", Alg.REDUCE_LTR, lambda P: 0),
}
MAX_BYTE = {"e4m3": 0x7E, "e5m2": 0x7B}  # the largest finite value, positive


@functools.lru_cache(maxsize=None)
def inputs(kind, P, n=N_FUSED, seed=7, finite=False):
    """Random non-NaN element bytes, per-block scales from 120..134 per peer. Shared and never modified: copy first."""
    xs, es = MX.random_inputs(kind, n, P, seed, finite=finite)
    for a in xs + es:
        a.setflags(write=False)
    return tuple(xs), tuple(es)


def cut(xs, es, n):
    return [x[:n] for x in xs], [e[:MX.blocks(n)] for e in es]


def bucket(bits, dtype, offset=0):
    bits = np.asarray(bits, np.uint8)
    b = Bucket(bits.size + offset, dtype)
    b.upload(np.concatenate([np.zeros(offset, np.uint8), bits]))
    return b.view(offset, bits.size) if offset else b


def out_buckets(n, kind, out, offset=0):
    """Buckets for the result and its scales, holding other values beforehand."""
    if out == "f32":
        b = Bucket(n, DType.F32)
        b.upload(np.full(n, 1.5, np.float32))
        return b, None
    return bucket(np.full(n, 0x55, np.uint8), DT[kind], offset), bucket(np.full(MX.blocks(n), 0x11, np.uint8), DType.F8E8M0, offset)


def read(o, osc, out):
    return (o.numpy().view(np.float32), None) if out == "f32" else (o.numpy(), osc.numpy())


def run(alg, kind, xs, es, op, out, root=0, offset=0, scale_offset=1, stream=None):
    """One call on fresh buckets. The scale arrays sit at an odd address unless told otherwise: any alignment."""
    n = xs[0].size
    ins = [bucket(x, DT[kind], offset) for x in xs]
    scs = [bucket(e, DType.F8E8M0, scale_offset) for e in es]
    o, osc = out_buckets(n, kind, out, offset)
    fmi_amd.reduce_tree_mx(OP[op], alg, o, osc, ins, scs, rank=root, stream=stream)
    fmi_amd.sync()
    return read(o, osc, out)


def check(name, kind, xs, es, op, out, offset=0, what=""):
    family, alg, root_of = ALGS[name]
    root = root_of(len(xs))
    want, want_sc = MX.expected_mx(family, kind, xs, es, op, out, root)
    got, got_sc = run(alg, kind, xs, es, op, out, root, offset)
    MX.assert_mx(got, got_sc, want, want_sc, kind, out, f"{what} {kind} {name} {op} P={len(xs)} n={xs[0].size} out={out}")
    return got, got_sc


# ---- 1. the fused kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["same", "f32"])
@pytest.mark.parametrize("P", [2, 3, 8, 16])
@pytest.mark.parametrize("name", list(ALGS))
@pytest.mark.parametrize("kind", F.KINDS)
def test_fused(device, kind, name, P, out):
    """The f32 output pins the order of the sum and the scale decode; the 8-bit one the block amax, the scale byte and
    the narrowing. SUM everywhere, the mean too at P = 3 and 8."""
    xs, es = inputs(kind, P)
    for n in THREE_SIZES:
        for op in (("sum", "avg") if P in (3, 8) else ("sum",)):
            check(name, kind, *cut(xs, es, n), op, out)


@pytest.mark.parametrize("out", ["same", "f32"])
@pytest.mark.parametrize("kind", F.KINDS)
def test_fused_every_size(device, kind, out):
    """P = 8 at every size: nothing but a ragged block (1, 31), one whole block (32), a block and a ragged one (33, 48,
    63), two blocks (64), more than a tile, three tiles. E5M2 once more without its inf bytes, which decide most blocks
    of an 8-peer sum otherwise."""
    for finite in ((False, True) if kind == "e5m2" else (False,)):
        xs, es = inputs(kind, 8, finite=finite)
        for n in SIZES:
            for name in ALGS:
                check(name, kind, *cut(xs, es, n), "sum", out, what=f"finite={finite}")
            check("allreduce", kind, *cut(xs, es, n), "avg", out, what=f"finite={finite}")


@pytest.mark.parametrize("policy", [0, 2])
def test_fused_both_access_policies(device, policy):
    """The global (0) and the buffer (2) accesses at peer counts the default would send the other way."""
    fmi_amd.tune_set(Tune.FUSED_POLICY, policy)
    try:
        for kind in F.KINDS:
            for P in (3, 8):
                xs, es = inputs(kind, P, finite=True)
                for n in (N_TILE, N_FUSED):
                    for out in ("same", "f32"):
                        check("allreduce", kind, *cut(xs, es, n), "sum", out, what=f"policy {policy}")
    finally:
        fmi_amd.tune_set(Tune.FUSED_POLICY, 1)


# ---- 2. decided blocks -----------------------------------------------------------------------------------------------
# block 0, block 129 (lane groups 258 / 259: the second tile), the ragged last block 131 (17 elements)
PLACES = (0, 129, 131)


def _base(kind, P=3):
    xs, es = inputs(kind, P, finite=True)
    xs, es = cut(xs, es, N_TILE)
    return [x.copy() for x in xs], [e.copy() for e in es]


def _span(b, n=N_TILE):
    return slice(32 * b, min(32 * b + 32, n))


@pytest.mark.parametrize("kind", F.KINDS)
def test_decided_blocks(device, kind):
    emax = MX.EMAX[kind]
    # E4M3: 0x3E = 1.75 sits on the threshold mantissa 0x600000 (no bump), 0x3F = 1.875 is above it (bump).
    # E5M2 has two mantissa bits: 0x3E = 1.5 is below the threshold and 0x3F = 1.75 sits ON it, neither bumps; no E5M2
    # byte lies above it within a binade, so the bump comes from a sum: 1.75 + 0.125 (0x30) = 1.875.
    on, below_or_above = 0x3F if kind == "e5m2" else 0x3E, 0x3E if kind == "e5m2" else 0x3F
    cases = {}

    def case(name, edit, want_e, want_q=None):
        xs, es = _base(kind)
        for b in PLACES:
            edit(xs, es, b)
        cases[name] = (xs, es, want_e, want_q)

    def nan_scale(xs, es, b):
        es[1][b] = 255
    case("a peer's scale byte is 255", nan_scale, 255, 0x7F)

    def zeros(xs, es, b):
        for x in xs:
            x[_span(b)] = 0
    case("an all-zero block", zeros, 0, 0)

    def overflow(xs, es, b):
        for x, e in zip(xs, es):
            x[_span(b)] = MAX_BYTE[kind]
            e[b] = 254
    case("scale 254 and the largest elements: S is inf", overflow, 255, 0x7F)

    def tiny(xs, es, b):
        for p, (x, e) in enumerate(zip(xs, es)):
            x[_span(b)] = 0x01  # the smallest subnormal
            e[b] = p            # scales 0, 1, 2 (and 3 below)
    case("scales 0..3 and the smallest subnormal elements: S is an f32 subnormal", tiny, 0)

    def single(byte):
        def edit(xs, es, b):
            for x, e in zip(xs, es):
                x[_span(b)] = 0
                e[b] = 127
            xs[0][_span(b).start + 5] = byte
        return edit
    case("the tie: 1.75, mantissa 0x600000, no bump", single(on), 127 - emax)
    if kind == "e4m3":
        case("1.875: above the threshold, a bump", single(below_or_above), 127 - emax + 1)
    else:
        case("1.5: below the threshold, no bump", single(below_or_above), 127 - emax)

        def summed(xs, es, b):
            single(on)(xs, es, b)
            xs[1][_span(b).start + 5] = 0x30  # 0.125
        case("1.75 + 0.125 = 1.875: a bump", summed, 127 - emax + 1)

    for name, (xs, es, want_e, want_q) in cases.items():
        if "subnormal" in name:
            xs.append(xs[0].copy()), es.append(es[0].copy())
            for b in PLACES:
                es[3][b] = 3
            S = MX.values("allreduce", kind, xs, es)
            for b in PLACES:
                assert (np.abs(S[_span(b)]) < np.float32(2.0 ** -126)).all() and (S[_span(b)] != 0).all(), name
        got, got_sc = check("allreduce", kind, xs, es, "sum", "same", what=name)
        for b in PLACES:
            assert got_sc[b] == want_e, (name, b, int(got_sc[b]), want_e)
            if want_q is not None:
                assert (got[_span(b)] == want_q).all(), (name, b)
        # the block's neighbours are ordinary blocks
        assert got_sc[1] not in (0, 255) and got_sc[130] not in (0, 255), name
        check("reduce_ltr", kind, xs, es, "sum", "f32", what=name)


# ---- 3. block independence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", [32 * 5 + 3, 32 * 5 + 20, 32 * 131 + 5, 4095],
                         ids=["first lane group", "second lane group", "ragged block", "last block of a tile"])
@pytest.mark.parametrize("kind", F.KINDS)
def test_a_huge_value_changes_its_own_block_only(device, kind, where):
    """Every peer holds the largest finite value at one position of a bucket whose other elements are below 1: that
    block's scale byte rises, its elements change, and no other block's byte or element does."""
    xs, es = _base(kind)
    small = np.flatnonzero(np.abs(F.widen(np.arange(256, dtype=np.uint8), kind)) < 1).astype(np.uint8)
    xs = [small[x.astype(np.int64) % small.size] for x in xs]
    base, base_sc = check("allreduce", kind, xs, es, "sum", "same", what="base")
    for x in xs:
        x[where] = MAX_BYTE[kind]
    got, got_sc = check("allreduce", kind, xs, es, "sum", "same", what=f"huge at {where}")
    b = where // 32
    assert got_sc[b] > base_sc[b], (int(got_sc[b]), int(base_sc[b]))
    others = np.ones(N_TILE, bool)
    others[_span(b)] = False
    assert np.array_equal(got[others], base[others])
    assert np.array_equal(np.delete(got_sc, b), np.delete(base_sc, b))
    assert not np.array_equal(got[_span(b)], base[_span(b)])


# ---- 4. quantize / dequantize -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", F.KINDS)
def test_dequantize_every_byte_under_every_scale(device, kind):
    """256 bytes x 256 scales: scale s holds blocks 8 s .. 8 s + 7, which hold the 256 bytes. To f32 (exact) and to
    bf16 (one rounding)."""
    q = np.tile(np.arange(256, dtype=np.uint8), 256)
    e = np.repeat(np.arange(256, dtype=np.uint8), 8)
    v = MX.dequant(q, e, kind)
    src, sc = bucket(q, DT[kind]), bucket(e, DType.F8E8M0)
    d32, d16 = Bucket(q.size, DType.F32), Bucket(q.size, DType.BF16)
    fmi_amd.mx_dequantize(d32, src, sc)
    fmi_amd.mx_dequantize(d16, src, sc)
    fmi_amd.sync()
    MX.assert_f32_bits(d32.numpy(), v, f"{kind} -> f32")
    H.assert_bits(d16.numpy(), H.narrow(v, "bf16"), "bf16", "sum", f"{kind} -> bf16")


@pytest.mark.parametrize("kind", F.KINDS)
def test_quantize_boundaries_and_every_bf16_pattern(device, kind):
    for name, S, src in (("boundary f32", F.boundary_f32(), None),
                         ("every bf16 pattern", H.widen(np.arange(65536, dtype=np.uint16), "bf16"), np.arange(65536, dtype=np.uint16))):
        want, want_sc = MX.quant(S, kind)
        if src is None:
            b = Bucket.from_numpy(S)
        else:
            b = Bucket(src.size, DType.BF16)
            b.upload(src)
        o, osc = out_buckets(S.size, kind, "same")
        fmi_amd.mx_quantize(o, osc, b)
        fmi_amd.sync()
        MX.assert_mx(o.numpy(), osc.numpy(), want, want_sc, kind, "same", f"{kind} quantize {name}")


@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("kind", F.KINDS)
def test_quantize_dequantize_unaligned_and_empty(device, kind, offset):
    n = N_TILE
    xs, es = cut(*inputs(kind, 1, finite=True), n)
    q, e = bucket(xs[0], DT[kind], offset), bucket(es[0], DType.F8E8M0, offset)
    wide = Bucket(n + offset, DType.F32).view(offset, n)  # offset elements: 4 and 12 bytes off 16-B alignment
    fmi_amd.mx_dequantize(wide, q, e)
    o, osc = out_buckets(n, kind, "same", offset)
    fmi_amd.mx_quantize(o, osc, wide)
    fmi_amd.sync()
    v = MX.dequant(xs[0], es[0], kind)
    MX.assert_f32_bits(wide.numpy(), v, "unaligned dequantize")
    want, want_sc = MX.quant(v, kind)
    MX.assert_mx(o.numpy(), osc.numpy(), want, want_sc, kind, "same", "unaligned quantize")
    # n = 0 succeeds
    lib = fmi_amd.load()
    assert lib.fmi_dev_mx_quantize(int(DT[kind]), o.ptr, osc.ptr, int(DType.F32), wide.ptr, 0, None) == 0
    assert lib.fmi_dev_mx_dequantize(int(DType.F32), wide.ptr, int(DT[kind]), q.ptr, e.ptr, 0, None) == 0


# ---- 5. beyond the fused kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["same", "f32"])
@pytest.mark.parametrize("P", [1, 17, 33])
@pytest.mark.parametrize("kind", F.KINDS)
def test_fallback_peer_counts(device, kind, P, out):
    """P = 1 (not a copy: it requantizes), 17 and 33 (f32 temporaries): the definition's bits."""
    xs, es = cut(*inputs(kind, P, finite=True), N_TILE)
    for name in ALGS:
        check(name, kind, xs, es, "sum", out, what="fallback")
    check("allreduce", kind, xs, es, "avg", out, what="fallback")
    check("allreduce", kind, *cut(xs, es, 31), "sum", out, what="fallback")


@pytest.mark.parametrize("out", ["same", "f32"])
@pytest.mark.parametrize("kind", F.KINDS)
def test_fallback_unaligned(device, kind, out):
    xs, es = cut(*inputs(kind, 5), N_TILE)
    for name in ALGS:
        check(name, kind, xs, es, "sum", out, offset=1, what="1-byte offset")
    check("reduce_ltr", kind, xs, es, "avg", out, offset=3, what="3-byte offset")


# ---- 6. in place ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, -1])
@pytest.mark.parametrize("kind", F.KINDS)
def test_in_place(device, kind, which):
    """out / out_scales are ins[p] / in_scales[p] themselves, p the first or the last peer."""
    P = 8
    xs, es = cut(*inputs(kind, P, finite=True), N_TILE)
    for name in ALGS:
        family, alg, root_of = ALGS[name]
        ins, scs = [bucket(x, DT[kind]) for x in xs], [bucket(e, DType.F8E8M0) for e in es]
        fmi_amd.reduce_tree_mx(Op.SUM, alg, ins[which], scs[which], ins, scs, rank=root_of(P))
        fmi_amd.sync()
        want, want_sc = MX.expected_mx(family, kind, xs, es, "sum", "same", root_of(P))
        MX.assert_mx(ins[which].numpy(), scs[which].numpy(), want, want_sc, kind, "same", f"in place {name} peer {which}")
        for p in range(1, P - 1):
            assert np.array_equal(ins[p].numpy(), xs[p]) and np.array_equal(scs[p].numpy(), es[p])


# ---- 7. graph capture ------------------------------------------------------------------------------------------------------
def test_graph_replay_reads_new_elements_and_scales(device):
    kind, P, n = "e4m3", 8, N_FUSED
    old, new = inputs(kind, P), inputs(kind, P, seed=8)
    ins, scs = [bucket(x, DT[kind]) for x in old[0]], [bucket(e, DType.F8E8M0) for e in old[1]]
    o, osc = out_buckets(n, kind, "same")
    fmi_amd.sync()
    st = Stream()
    g = Graph.capture(st, lambda: fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, o, osc, ins, scs, stream=st))
    try:
        for xs, es in (old, new):
            for b, a in zip(ins + scs, list(xs) + list(es)):
                b.upload(a)
            g.launch(st)
            st.sync()
            want, want_sc = MX.expected_mx("allreduce", kind, xs, es)
            MX.assert_mx(o.numpy(), osc.numpy(), want, want_sc, kind, "same", "graph replay")
    finally:
        g.destroy()
        st.destroy()


# ---- 8. the communicator: LOCAL transport, every rank compared ---------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("N", [2, 3, 8])
@pytest.mark.parametrize("kind", F.KINDS)
def test_comm_allreduce_mx(device, kind, N, ragged):
    from tests.test_gpu_comm import run_ranks

    n = 64 * N * 3 + (45 if ragged else 0)
    xs, es = MX.random_inputs(kind, n, N, seed=81, finite=True)

    def body(c, r):
        send, ssc, res = bucket(xs[r], DT[kind]), bucket(es[r], DType.F8E8M0), {}
        for out in ("same", "f32"):
            for op, ordered in (("sum", False), ("sum", True), ("avg", False)):
                recv, rsc = out_buckets(n, kind, out)
                c.allreduce_mx(OP[op], send, ssc, recv, rsc, ordered=ordered)
                fmi_amd.sync()
                res[out, op, ordered] = read(recv, rsc, out)
        res["send"] = (send.numpy(), ssc.numpy())
        return res

    res = run_ranks(N, body)
    for out in ("same", "f32"):
        for op, ordered in (("sum", False), ("sum", True), ("avg", False)):
            want, want_sc = MX.expected_mx("allreduce_ltr" if ordered else "allreduce", kind, xs, es, op, out)
            for r in range(N):
                got, got_sc = res[r][out, op, ordered]
                MX.assert_mx(got, got_sc, want, want_sc, kind, out, f"{kind} N={N} n={n} out={out} {op} ordered={ordered} rank {r}")
    for r in range(N):
        assert np.array_equal(res[r]["send"][0], xs[r]) and np.array_equal(res[r]["send"][1], es[r]), f"send of rank {r} was modified"


def test_one_rank_communicator_runs_the_p1_form(device):
    from tests.test_gpu_comm import run_ranks

    kind, n = "e5m2", 1000
    xs, es = MX.random_inputs(kind, n, 1, seed=85, finite=True)

    def body(c, r):
        recv, rsc = out_buckets(n, kind, "same")
        c.allreduce_mx(Op.SUM, bucket(xs[0], DT[kind]), bucket(es[0], DType.F8E8M0), recv, rsc)
        fmi_amd.sync()
        return recv.numpy(), rsc.numpy()

    got, got_sc = run_ranks(1, body)[0]
    want, want_sc = MX.expected_mx("allreduce", kind, xs, es)
    MX.assert_mx(got, got_sc, want, want_sc, kind, "same", "one rank")
    assert not np.array_equal(got_sc, es[0]), "P = 1 requantizes: random blocks do not keep their scale bytes"


# ---- 9. the Python layers ------------------------------------------------------------------------------------------------
def test_python_layers_refuse_wrong_buckets(device):
    xs, es = cut(*inputs("e4m3", 2), 64)
    ins, scs = [bucket(x, DType.F8E4M3) for x in xs], [bucket(e, DType.F8E8M0) for e in es]
    with pytest.raises(ValueError, match="in their dtype or in F32"):
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, Bucket(64, DType.BF16), Bucket(2, DType.F8E8M0), ins, scs)
    with pytest.raises(ValueError, match="scale bytes"):
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, Bucket(64, DType.F32), None, ins, [scs[0], Bucket(3, DType.F8E8M0)])
    with pytest.raises(ValueError, match="out_scales is missing"):
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, Bucket(64, DType.F8E4M3), None, ins, scs)
    with pytest.raises(fmi_amd.FmiError, match="scan algorithm"):
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.SCAN, Bucket(64, DType.F32), None, ins, scs)
    with pytest.raises(fmi_amd.FmiError, match="op 2 is not valid here"):
        fmi_amd.reduce_tree_mx(Op.MAX, Alg.ALLREDUCE, Bucket(64, DType.F32), None, ins, scs)


def test_torch_glue(device):
    """HipEngine.reduce_tree_mx on torch float8 device tensors with float8_e8m0fnu scale tensors (a child process: torch
    must be loaded before the library) equals the definition."""
    r = subprocess.run([sys.executable, "-u", "-m", "tests._mx_torch_worker"], cwd=ROOT, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0 and "mx torch glue ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
