"""Stochastic rounding on the GPU (fmi_dev_reduce_tree_mx_sr, fmi_dev_mx_quantize_sr, fmi_comm_allreduce_mx_sr), bit for
bit against tests/_mx_sr.py, scale bytes included, at E4M3, E5M2 and E2M1. Inputs come from the family on which the
rounding shows (tests/test_mx_sr_cpu.py asserts that there SR differs from round-to-nearest, and two seeds from each
other, on more than 5 % of the elements), so a kernel that rounds to nearest, ignores the seed or keys the bits by
thread cannot pass. Every output is guarded and poisoned (tests/_guard.py); inputs and the seed word are frozen."""
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
from tests import _mxfp4 as M4
from tests.test_gpu_fp8_scaled import N_FUSED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"e4m3": DType.F8E4M3, "e5m2": DType.F8E5M2, "e2m1": DType.F4E2M1}
OP = {"sum": Op.SUM, "avg": Op.AVG}
N_TILE = M4.N_TILE
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, N_TILE, N_FUSED)
THREE_SIZES = (33, N_TILE, N_FUSED)
ALGS = {
    "allreduce": ("allreduce", Alg.ALLREDUCE, lambda P: 0),
    "reduce_rootlast": ("reduce", Alg.REDUCE, lambda P: P - 1),
    "reduce_ltr": ("reduce_ltr", Alg.REDUCE_LTR, lambda P: 0),
}
SEED = 0x0123456789ABCDEF


@functools.lru_cache(maxsize=None)
def inputs(kind, P, n=N_FUSED):
    xs, es = SR.visible_inputs(kind, n, P)
    for a in xs + es:
        a.setflags(write=False)
    return tuple(xs), tuple(es)


def byte_offset(kind, nbytes):
    """A bucket `nbytes` bytes off 16-B alignment, in tests/_guard.py's element offsets."""
    return 2 * nbytes if kind == "e2m1" else nbytes


def frozen_elements(kind, xs, offset=0):
    n = xs[0].size
    return G.FrozenSet([SR.element_bytes(x, kind) for x in xs], DT[kind], byte_offset(kind, offset), n=n if kind == "e2m1" else None)


def seed_word(seed):
    return G.frozen([np.array([seed], np.uint64)], DType.U64)


def outputs(kind, want, want_sc, n, offset=0):
    """(elements, scale bytes) guarded outputs for one call, the scale bytes at an odd address: as many runs as the longer
    of the two poison choices needs."""
    runs = G.guarded_runs(SR.element_bytes(want, kind), n, DT[kind], byte_offset(kind, offset))
    sruns = G.guarded_runs(want_sc, MX.blocks(n), DType.F8E8M0, 1)
    for j in range(max(len(runs), len(sruns))):
        g, gs = runs[j % len(runs)], sruns[j % len(sruns)]
        if j >= len(runs):
            g.repoison()
        if j >= len(sruns):
            gs.repoison()
        yield g, gs


def assert_same(kind, g, gs, want, want_sc, n, what):
    """Guards, poison, then codes and scale bytes exactly (an odd E2M1 bucket's last high nibble is 0 in want's bytes)."""
    raw = g.read(SR.element_bytes(want, kind), what)
    got_sc = gs.read(want_sc, f"scales of {what}")
    bad = np.flatnonzero(got_sc != want_sc)
    assert bad.size == 0, f"{what}: scale bytes differ at blocks {bad[:8]}: got {got_sc[bad[:8]]}, want {want_sc[bad[:8]]}"
    if kind == "e2m1" and n % 2:
        assert raw[-1] >> 4 == 0, f"{what}: the last byte's unused high nibble is {raw[-1] >> 4:#x}, not 0"
    got = SR.codes_of(raw, kind, n)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {n} codes differ; first at {bad[:8]}: got {got[bad[:8]]}, want {want[bad[:8]]}"
    return got, got_sc


def check(kind, name, xs, es, op="sum", seed=SEED, first=32, offset=0, what=""):
    family, alg, root_of = ALGS[name]
    P, n = len(xs), xs[0].size
    root = root_of(P)
    what = f"{what} {kind} {name} {op} P={P} n={n} seed={seed:#x} first={first}"
    want, want_sc = SR.expected_sr(family, kind, xs, es, seed, first, op, root)
    ins, scs, word = frozen_elements(kind, xs, offset), G.frozen(list(es), DType.F8E8M0, 1), seed_word(seed)
    for g, gs in outputs(kind, want, want_sc, n, offset):
        fmi_amd.reduce_tree_mx(OP[op], alg, g.b, gs.b, ins.bs, scs.bs, rank=root, seed=word.bs[0], first=first)
        fmi_amd.sync()
        got = assert_same(kind, g, gs, want, want_sc, n, what)
    ins.assert_intact(what)
    scs.assert_intact(f"scales of {what}")
    word.assert_intact(f"seed of {what}")
    return got


# ---- 1. the fused kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 3, 8, 16])
@pytest.mark.parametrize("name", list(ALGS))
@pytest.mark.parametrize("kind", SR.KINDS)
def test_fused(device, kind, name, P):
    xs, es = inputs(kind, P)
    for n in THREE_SIZES:
        for op in ("sum", "avg"):
            check(kind, name, *SR.cut(xs, es, n), op)


@pytest.mark.parametrize("kind", SR.KINDS)
def test_fused_every_size(device, kind):
    xs, es = inputs(kind, 8)
    for n in SIZES:
        for name in ALGS:
            check(kind, name, *SR.cut(xs, es, n))
        check(kind, "allreduce", *SR.cut(xs, es, n), "avg")


@pytest.mark.parametrize("policy", [0, 2])
@pytest.mark.parametrize("kind", SR.KINDS)
def test_fused_both_access_policies(device, kind, policy):
    before = fmi_amd.tune_get(Tune.FUSED_POLICY)
    fmi_amd.tune_set(Tune.FUSED_POLICY, policy)
    try:
        for P in (3, 8):
            xs, es = inputs(kind, P)
            for n in (N_TILE, N_FUSED):
                check(kind, "allreduce", *SR.cut(xs, es, n), what=f"policy {policy}")
    finally:
        fmi_amd.tune_set(Tune.FUSED_POLICY, before)


@pytest.mark.parametrize("kind", SR.KINDS)
def test_first_and_seeds(device, kind):
    """Every `first` of the CPU tests (the last one crosses q = 2^32) and every seed; the results differ between seeds."""
    xs, es = SR.cut(*inputs(kind, 8), N_TILE)
    seen = []
    for first in SR.FIRSTS:
        for seed in SR.SEEDS:
            got, _ = check(kind, "allreduce", xs, es, seed=seed, first=first)
            seen.append(got)
    assert all((a != b).mean() > 0.05 for a, b in zip(seen, seen[1:])), "neighbouring (seed, first) pairs give the same rounding"


@pytest.mark.parametrize("kind", SR.KINDS)
def test_split_calls_equal_one_call(device, kind):
    """A bucket reduced in two calls, split at a multiple of 32 inside the tile, the second at first + split."""
    xs, es = SR.cut(*inputs(kind, 8), N_TILE)
    first = 64
    whole, whole_sc = SR.expected_sr("allreduce", kind, xs, es, SEED, first)
    for split in (32, 4096 + 96):
        a, a_sc = check(kind, "allreduce", [x[:split] for x in xs], [e[:split // 32] for e in es], first=first, what="head")
        b, b_sc = check(kind, "allreduce", [x[split:] for x in xs], [e[split // 32:] for e in es], first=first + split, what="tail")
        assert np.array_equal(np.concatenate([a, b]), whole) and np.array_equal(np.concatenate([a_sc, b_sc]), whole_sc), split


# ---- 2. beyond the fused kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 17, 33])
@pytest.mark.parametrize("kind", SR.KINDS)
def test_fallback_peer_counts(device, kind, P):
    xs, es = SR.cut(*inputs(kind, P), N_TILE)
    for name in ALGS:
        check(kind, name, xs, es, what="fallback")
    check(kind, "allreduce", xs, es, "avg", what="fallback")
    check(kind, "allreduce", *SR.cut(xs, es, 31), what="fallback")


@pytest.mark.parametrize("kind", SR.KINDS)
def test_fallback_unaligned(device, kind):
    """Element buckets one byte off alignment: the same definition, so the same bits as the fused kernel at offset 0."""
    xs, es = SR.cut(*inputs(kind, 3), N_TILE)
    fused = check(kind, "allreduce", xs, es)
    for name in ALGS:
        got = check(kind, name, xs, es, offset=1, what="1-byte offset")
        if name == "allreduce":
            assert np.array_equal(got[0], fused[0]) and np.array_equal(got[1], fused[1])
    check(kind, "reduce_ltr", xs, es, "avg", offset=1, what="1-byte offset")


# ---- 3. mx_quantize with a seed ------------------------------------------------------------------------------------------
def quantize(kind, S, seed, first, src=None, src_dtype=DType.F32, offset=0, what=""):
    """S: the f32 values; src: their storage bits where the source is not f32."""
    n = S.size
    want, want_sc = SR.quant_sr(S, kind, seed, first)
    wide = G.frozen([S if src is None else src], src_dtype)
    word = seed_word(seed)
    for g, gs in outputs(kind, want, want_sc, n, offset):
        fmi_amd.mx_quantize(g.b, gs.b, wide.bs[0], seed=word.bs[0], first=first)
        fmi_amd.sync()
        got = assert_same(kind, g, gs, want, want_sc, n, what)
    wide.assert_intact(what)
    word.assert_intact(f"seed of {what}")
    return got


@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("src", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("kind", SR.KINDS)
def test_quantize_sources_and_offsets(device, kind, src, offset):
    n = N_TILE  # odd
    xs, es = SR.cut(*inputs(kind, 8), n)
    S = SR.values("allreduce", kind, xs, es)
    bits = None
    if src != "f32":
        with np.errstate(all="ignore"):
            bits = H.narrow(S, src)
        S = H.widen(bits, src)
    for first in (0, 2 ** 35 - 64):
        quantize(kind, S, SEED, first, bits, {"f32": DType.F32, "f16": DType.F16, "bf16": DType.BF16}[src], offset,
                 f"quantize {kind} from {src} at byte offset {offset}")
    quantize(kind, S[:31], 1, 32, None if bits is None else bits[:31], {"f32": DType.F32, "f16": DType.F16, "bf16": DType.BF16}[src], offset,
             "quantize a ragged block")


@pytest.mark.parametrize("kind", SR.KINDS)
def test_quantize_exhaustive_rounding(device, kind):
    """Every grid value, every midpoint and both f32 neighbours of each, both signs, in blocks whose first element is the
    largest finite element (y is the value itself), at three block scales under four seeds; with the f32 boundary set's
    blocks, NaN / inf blocks and all-zero blocks after them."""
    v = SR.exhaustive_values(kind)
    S = np.concatenate([SR.pinned_blocks(v, kind, 2.0 ** k) for k in (-3, 0, 5)] +
                       [np.zeros(64, np.float32), np.array([np.nan, 1, 2] + [0.5] * 29 + [np.inf] + [1] * 31, np.float32)])
    for seed in SR.SEEDS:
        got, got_sc = quantize(kind, S, seed, 0, what=f"exhaustive {kind} seed {seed:#x}")
        assert (got_sc[-2:] == 255).all() and (got[-64:] == (0 if kind == "e2m1" else 0x7F)).all()
    # a grid value is never moved: the codes of the grid values equal round-to-nearest's under every seed (asserted on
    # the definition in tests/test_mx_sr_cpu.py; the comparison above pins the device to it)


def test_quantize_statistics(device):
    """E2M1, n = 65,536, every 32nd element 6.0 (the block scale stays 2^0), the rest 2.3, 2.5 or 1.03125: the share rounded
    up lies within 4 sigma of t = 0.3, 0.5, 0.0625 under each seed (on the definition: within 1.6 sigma)."""
    n = 65536
    for value, t, lo_code in ((2.3, None, 4), (2.5, 0.5, 4), (1.03125, 0.0625, 2)):
        S = np.full(n, value, np.float32)
        S[0::32] = 6.0
        if t is None:
            t = (float(np.float32(2.3)) - 2.0) / 1.0  # fl32(2.3) is what is rounded: 0.3 to 2^-23
        body = np.arange(n) % 32 != 0
        for seed in SR.SEEDS:
            got, _ = quantize("e2m1", S, seed, 0, what=f"statistics {value} seed {seed:#x}")
            assert set(np.unique(got[body])) <= {lo_code, lo_code + 1}
            share = (got[body] == lo_code + 1).mean()
            assert body.sum() == 63488 and abs(share - t) <= 4 * np.sqrt(t * (1 - t) / 63488), (value, seed, share, t)


# ---- 4. in place ---------------------------------------------------------------------------------------------------------
def plain_bucket(raw, dtype, n=None):
    raw = np.asarray(raw, np.uint8)
    b = Bucket(raw.size if n is None else n, dtype)
    b.upload(raw)
    return b


@pytest.mark.parametrize("which", [0, -1])
@pytest.mark.parametrize("kind", SR.KINDS)
def test_in_place(device, kind, which):
    P, n = 8, N_TILE
    xs, es = SR.cut(*inputs(kind, P), n)
    word = seed_word(SEED)
    for name, (family, alg, root_of) in ALGS.items():
        ins = [plain_bucket(SR.element_bytes(x, kind), DT[kind], n) for x in xs]
        scs = [plain_bucket(e, DType.F8E8M0) for e in es]
        fmi_amd.reduce_tree_mx(Op.SUM, alg, ins[which], scs[which], ins, scs, rank=root_of(P), seed=word.bs[0], first=64)
        fmi_amd.sync()
        want, want_sc = SR.expected_sr(family, kind, xs, es, SEED, 64, "sum", root_of(P))
        assert np.array_equal(SR.codes_of(ins[which].numpy(), kind, n), want), f"in place {kind} {name} peer {which}"
        assert np.array_equal(scs[which].numpy(), want_sc), f"in place scales {kind} {name} peer {which}"
        for p in range(1, P - 1):
            assert np.array_equal(ins[p].numpy(), SR.element_bytes(xs[p], kind)) and np.array_equal(scs[p].numpy(), es[p])
    word.assert_intact("seed")


# ---- 5. graph capture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SR.KINDS)
def test_graph_replay_reads_the_new_seed(device, kind):
    P, n = 8, N_FUSED
    xs, es = inputs(kind, P)
    ins, scs = frozen_elements(kind, xs), G.frozen(list(es), DType.F8E8M0, 1)
    word = Bucket.from_numpy(np.array([SR.SEEDS[1]], np.uint64))
    wants = [SR.expected_sr("allreduce", kind, xs, es, seed, 32) for seed in SR.SEEDS[1:3]]
    (g, gs), = list(outputs(kind, wants[0][0], wants[0][1], n))[:1]
    fmi_amd.sync()
    st = Stream()
    graph = Graph.capture(st, lambda: fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, g.b, gs.b, ins.bs, scs.bs, seed=word, first=32, stream=st))
    try:
        seen = []
        for seed, (want, want_sc) in zip(SR.SEEDS[1:3], wants):
            word.upload(np.array([seed], np.uint64))
            g.repoison(), gs.repoison()
            graph.launch(st)
            st.sync()
            raw = g.read(None, "graph replay")
            got_sc = gs.read(None, "graph replay scales")
            got = SR.codes_of(raw, kind, n)
            assert np.array_equal(got_sc, want_sc) and np.array_equal(got, want), f"graph replay {kind} seed {seed:#x}"
            seen.append(got)
        assert (seen[0] != seen[1]).mean() > 0.05, "the replay did not read the new seed"
    finally:
        graph.destroy()
        st.destroy()
    ins.assert_intact("graph")


# ---- 6. the communicator: LOCAL transport, every rank compared -------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("N", [2, 3, 8])
@pytest.mark.parametrize("kind", SR.KINDS)
def test_comm_allreduce_mx_sr(device, kind, N, ragged):
    from tests.test_gpu_comm import run_ranks

    n = 192 * N + (45 if ragged else 0)
    xs, es = SR.cut(*inputs(kind, N), n)
    first = 64
    cases = (("sum", False), ("sum", True), ("avg", False))
    wants = {c: SR.expected_sr("allreduce_ltr" if c[1] else "allreduce", kind, xs, es, SEED, first, c[0]) for c in cases}

    def body(c, r):
        send, ssc, word, res = frozen_elements(kind, [xs[r]]), G.frozen([es[r]], DType.F8E8M0, 1), seed_word(SEED), {}
        for case in cases:
            want, want_sc = wants[case]
            for g, gs in outputs(kind, want, want_sc, n):
                c.allreduce_mx(OP[case[0]], send.bs[0], ssc.bs[0], g.b, gs.b, ordered=case[1], seed=word.bs[0], first=first)
                fmi_amd.sync()
                res[case] = (g.read(SR.element_bytes(want, kind), f"rank {r}"), gs.read(want_sc, f"rank {r} scales"))
        send.assert_intact(f"send of rank {r}"), ssc.assert_intact(f"send scales of rank {r}"), word.assert_intact("seed")
        return res

    res = run_ranks(N, body)
    for case in cases:
        want, want_sc = wants[case]
        for r in range(N):
            raw, got_sc = res[r][case]
            assert np.array_equal(got_sc, want_sc), f"{kind} N={N} n={n} {case} rank {r}: scale bytes"
            assert np.array_equal(SR.codes_of(raw, kind, n), want), f"{kind} N={N} n={n} {case} rank {r}"


@pytest.mark.parametrize("kind", SR.KINDS)
def test_one_rank_communicator_runs_the_p1_form(device, kind):
    from tests.test_gpu_comm import run_ranks

    n = 1001
    xs, es = SR.cut(*inputs(kind, 1), n)
    want, want_sc = SR.expected_sr("allreduce", kind, xs, es, SEED, 64)

    def body(c, r):
        send, ssc, word = frozen_elements(kind, xs), G.frozen(list(es), DType.F8E8M0, 1), seed_word(SEED)
        for g, gs in outputs(kind, want, want_sc, n):
            c.allreduce_mx(Op.SUM, send.bs[0], ssc.bs[0], g.b, gs.b, seed=word.bs[0], first=64)
            fmi_amd.sync()
            assert_same(kind, g, gs, want, want_sc, n, "one rank")
        return True

    assert run_ranks(1, body) == [True]


# ---- 7. the upper layers ---------------------------------------------------------------------------------------------------
def test_python_argument_checks(device):
    xs, es = SR.cut(*inputs("e2m1", 2), 64)
    ins, scs = frozen_elements("e2m1", xs), G.frozen(list(es), DType.F8E8M0, 1)
    out, out_sc, wide = Bucket(64, DType.F4E2M1), Bucket(2, DType.F8E8M0), Bucket(64, DType.F32)
    with pytest.raises(ValueError, match="U64 bucket of one element"):
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, out, out_sc, ins.bs, scs.bs, seed=Bucket(2, DType.U64))
    with pytest.raises(ValueError, match="U64 bucket of one element"):
        fmi_amd.mx_quantize(out, out_sc, wide, seed=Bucket(1, DType.I64))
    word = seed_word(1)
    with pytest.raises(ValueError, match="nothing to round"):
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, wide, None, ins.bs, scs.bs, seed=word.bs[0])
    with pytest.raises(fmi_amd.FmiError, match="multiple of 32"):
        fmi_amd.reduce_tree_mx(Op.SUM, Alg.ALLREDUCE, out, out_sc, ins.bs, scs.bs, seed=word.bs[0], first=16)


def test_torch_glue(device):
    """HipEngine.reduce_tree_mx(seed=...) on torch tensors of the three element types (a child process: torch must be
    loaded before the library) equals the definition."""
    r = subprocess.run([sys.executable, "-u", "-m", "tests._mx_sr_torch_worker"], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and r.stdout.count("mx sr torch glue ok") == 3, (r.stdout[-3000:], r.stderr[-3000:])
