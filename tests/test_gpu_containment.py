"""Containment on the MI355X ("Containment"): an entry point writes exactly the bytes of its outputs and no
byte of an input it does not own. Every case here runs into guarded, poisoned outputs and from frozen inputs
(tests/_guard.py): the result is compared bit for bit with the oracle or definition the project already uses for that
call, no output element may still hold the poison, every guard byte before and after every output and input must be
unchanged, and every input the call does not own must come back as it went up.

Shapes are the smallest at which each store path exists. With W = 16 / itemsize lanes per 16-B group: 1, W - 1, W, W + 1
(the scalar tail alone, one lane group, a group and a tail) and 515 W + (W - 1): two whole 256-thread tiles, a partial
tile of three lane groups and the longest tail. Beyond 64 peers: 2 W + (W - 1), and the 515-group size at f32 alone.
Placements: everything 16-B aligned; the output one element off alignment; the output aligned and one input one
element off. Peer counts come from fmi_schedule.h's constants.

What runs (sizes are the five above unless stated; "3 places" = the three placements, "2 places" = aligned and out + 1):
  pairwise            reduce_pair, combine, reduce_pair_batch: all 14 element types x 4 ops x 3 places; launch variants
                      0..4 (unroll 4, 256 threads) at f32 / i8, 515 W + W - 1 and 16 tiles + W + 1, 3 places
  reduce_tree         allreduce ranks 0 / P - 1, reduce roots 0 / P - 1, reduce_ltr; P = 1 2 3 16 17 31 32 33 48 128 129 143
                      144 257; f32 i64 f16 bf16 at every P, f64 i32 at P <= 16; sum max, all four ops at P = 3, 16; 3 places;
                      P > 64: n = 3 W - 1, and 2063 at f32
  scan_peers          scan, scan_ltr, all P outputs guarded: the same P, types, ops, sizes and places
  FUSED_POLICY        0 and 2 at P = 3, 16: f32 i64 f16 bf16, sum max, aligned, trees and scans
  BLOCKS_ONE_PASS 0   P = 17 33 48 129 144: f32 bf16, sum max, 2 places, trees and scans
  FMI_ACC_F32         f16 bf16 e4m3 e5m2, sum prod, P = 2 16 17 33, 2 places, trees and scans
  FMI_OP_AVG          f32 f64 f16 bf16, f16 / bf16 also with FMI_ACC_F32; P = 1 3 16 17; 2 places; mean_scale alone at P = 3, 7
  FP8 plain           e4m3 e5m2, sum max, P = 3 17, 2 places, trees and scans
  reduce_tree_scaled  e4m3 e5m2 to the same type and to f32, P = 2 8 16 17, every bucket aligned and one element off; amax
                      alone in a guarded region, scale arrays frozen
  MXFP8               mx_dequantize / mx_quantize (f32 f16 bf16; n = 1 31 32 33 8255; aligned and off by one),
                      reduce_tree_mx (P = 2 16 17; n = 1 31 33 8255; to the same type and to f32; aligned and off by one);
                      MXFP4: tests/test_gpu_mxfp4.py (Out), which guards every output of its own
  convert             every ordered pair of f32 f16 bf16 e4m3 e5m2, dst aligned and off by one
  fill_synthetic      all 14 types, peers 0 and 5, aligned and off by one
  d2d, memset         16, 262143, 262144 + 5 bytes (offsets 0/0, 3/0, 0/1); memset 1 15 16 17 8255 262149 bytes, 2 offsets
  communicator        LOCAL transport, N = 2, 3: allreduce (plain, ordered), reduce, scan (f32, n = 2063, sum max);
                      allreduce_scaled, allreduce_mx (n = 8255); bcast, gather, scatter (i64, n = 1033); every recv guarded,
                      every send frozen"""
import functools
import os
import re

import numpy as np
import pytest

import fmi_amd
from fmi_amd import Alg, DType, Op, Tune
from oracle import fmi_oracle as orc
from tests import _avg as AV
from tests import _fp8 as F
from tests import _fp8_scaled as FS
from tests import _guard as G
from tests import _half as H
from tests import _half_acc as A
from tests import _mx as MX
from tests.test_gpu_parity import assert_bit_equal
from tests.test_gpu_parity import inputs as core_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {"sum": Op.SUM, "prod": Op.PROD, "max": Op.MAX, "min": Op.MIN}


def _constant(header, name):
    text = open(os.path.join(ROOT, "fmi_amd", "csrc", header)).read()
    return int(re.search(r"constexpr int %s\s*=\s*(\d+)\s*;" % name, text).group(1))


FUSED = _constant("fmi_schedule.h", "kMaxFusedPeers")               # 16: the fused single-pass kernels
WIDE = _constant("fmi_schedule.h", "kMaxFusedAllreducePeers")       # 31: the wide units' last P
PREFOLD = _constant("fmi_schedule.h", "kFusedInputCap")             # 32: the pre-fold block
SCAN_BLOCK = _constant("fmi_schedule.h", "kScanBlock")              # 16
ONE_PASS = _constant("fmi_internal.h", "kMaxOnePassScanBlocks") * SCAN_BLOCK  # 128: one pass against superblocks
SCAN_ONE_PASS = ONE_PASS + SCAN_BLOCK - 1                           # 143: the scan's one-pass limit
# 1, 2, 3, 16 | 17, 31 | 32, 33, 48 | 128, 129 | 143, 144 | 257 (two levels of blocks)
PEERS = [1, 2, 3, FUSED, FUSED + 1, WIDE, PREFOLD, PREFOLD + 1, 3 * FUSED, ONE_PASS, ONE_PASS + 1, SCAN_ONE_PASS,
         SCAN_ONE_PASS + 1, FUSED * FUSED + 1]
MANY = 64  # beyond this no case grows with P


# ---- element types ---------------------------------------------------------------------------------------------------
class Kind:
    """One element type: its DType, host inputs (raw bit patterns for the 16- and 8-bit floats), the oracle's combine
    and the project's own comparison for it."""

    def __init__(self, name, dtype, np_dtype=None):
        self.name, self.dtype, self.np = name, dtype, np_dtype
        self.size = G.element_bytes(dtype)
        self.W = 16 // self.size

    def inputs(self, n, peer, seed=7):
        if self.name in H.KINDS:
            return H.inputs(self.name, n, seed=seed, peer=peer)
        if self.name in F.KINDS:
            return F.synthetic(self.name, n, seed, peer)
        return core_inputs(self.np, n, peer, seed=seed)

    def f(self, op):
        if self.name in H.KINDS:
            return H.combiner(op, self.name)
        if self.name in F.KINDS:
            return F.combiner(op, self.name)
        return orc.OPS[op]

    def bits(self, got):
        """A downloaded body in the form the comparison takes."""
        if self.name in H.KINDS:
            return np.asarray(got).view(np.uint16)
        return np.asarray(got)

    def same(self, got, want, op, what):
        got = self.bits(got)
        if self.name in H.KINDS:
            H.assert_bits(got, want, self.name, "sum" if op == "avg" else op, what)
        elif self.name in F.KINDS:
            F.assert_bits(got, want, self.name, what)
        else:
            assert_bit_equal(got, np.asarray(want, self.np), what)

    def sizes(self, P=1):
        W = self.W
        if P > MANY:
            return [3 * W - 1] + ([516 * W - 1] if self.name == "f32" else [])
        return [1, W - 1, W, W + 1, 516 * W - 1] if W > 2 else [1, W, W + 1, 516 * W - 1]  # f64 / i64: W - 1 = 1


KINDS = {k.name: k for k in [
    Kind("f32", DType.F32, np.float32), Kind("f64", DType.F64, np.float64), Kind("i32", DType.I32, np.int32),
    Kind("i64", DType.I64, np.int64), Kind("u32", DType.U32, np.uint32), Kind("u64", DType.U64, np.uint64),
    Kind("i8", DType.I8, np.int8), Kind("u8", DType.U8, np.uint8), Kind("i16", DType.I16, np.int16),
    Kind("u16", DType.U16, np.uint16), Kind("f16", DType.F16), Kind("bf16", DType.BF16), Kind("e4m3", DType.F8E4M3),
    Kind("e5m2", DType.F8E5M2)]}
PLACES = ("aligned", "out+1", "in+1")


def place(P, where):
    """(the output's element offset, every input's)."""
    ins = [0] * P
    if where == "in+1":
        ins[P // 2] = 1
    return (1 if where == "out+1" else 0), ins


@functools.lru_cache(maxsize=None)
def peer_inputs(kind, n, P, seed=7):
    xs = tuple(KINDS[kind].inputs(n, p, seed) for p in range(P))
    for x in xs:
        x.setflags(write=False)
    return xs


@functools.lru_cache(maxsize=None)
def expected(mode, kind, op, family, n, P, root=0):
    """The oracle's value for one call, computed once and left unchanged: a list per rank for allreduce and the scans,
    one array for reduce (at `root`) and reduce_ltr. mode: "plain", "acc" (FMI_ACC_F32), "avg", "avg_acc"."""
    xs, k = list(peer_inputs(kind, n, P)), KINDS[kind]
    with np.errstate(all="ignore"):
        if mode in ("avg", "avg_acc"):
            return AV.expected_avg(family, kind, xs, mode == "avg_acc", root)
        if mode == "acc":
            w = (A if kind in H.KINDS else F).expected_acc(family, kind, op, xs, root)
            return w[0] if family == "reduce" else w
        f = k.f(op)
        if family == "allreduce":
            return orc.allreduce(xs, f)[0]
        if family == "reduce":
            return orc.reduce(xs, f, root=root)[0]
        if family == "reduce_ltr":
            return orc.reduce(xs, f, root=0, commutative=False, associative=False)[0]
        if family == "scan":
            return orc.scan(xs, f)[0]
        if family == "scan_ltr":
            return orc.scan(xs, f, commutative=False, associative=False)[0]
    raise ValueError(family)


def into_guarded(k, want, n, off, launch, op, what, count=None):
    """`launch(buckets)` into guarded, poisoned outputs: once, or once under each poison of a pair; `want`: the one
    expected body, or (count given) the list of the `count` bodies."""
    wants = [want] if count is None else list(want)
    for g in G.guarded_runs(wants, n, k.dtype, off, len(wants)):
        launch(g.bs)
        fmi_amd.sync()
        for j, got in enumerate(g.read_all(wants, what)):
            k.same(got, wants[j], op, f"{what} output {j}")


TREES = (("allreduce", Alg.ALLREDUCE, lambda P: sorted({0, P - 1})), ("reduce", Alg.REDUCE, lambda P: sorted({0, P - 1})),
         ("reduce_ltr", Alg.REDUCE_LTR, lambda P: [0]))
SCANS = (("scan", Alg.SCAN), ("scan_ltr", Alg.SCAN_LTR))


def run_trees(kind, op, P, n, where, mode="plain"):
    """allreduce at ranks 0 and P - 1, reduce at roots 0 and P - 1, reduce_ltr."""
    k, (out_off, in_offs) = KINDS[kind], place(P, where)
    ins = G.frozen(peer_inputs(kind, n, P), k.dtype, in_offs)
    acc, dev_op = mode in ("acc", "avg_acc"), (Op.AVG if mode.startswith("avg") else OPS[op])
    tag = f"{mode} {kind} {op} P={P} n={n} {where}"
    for family, alg, ranks in TREES:
        for r in ranks(P):
            want = expected(mode, kind, op, family, n, P, r if family == "reduce" else 0)
            want = want[r] if family == "allreduce" else want
            into_guarded(k, want, n, out_off,
                         lambda bs: fmi_amd.reduce_tree(dev_op, alg, bs[0], ins.bs, rank=r, accumulate_f32=acc),
                         op, f"{family} rank {r} {tag}")
    ins.assert_intact(f"trees {tag}")


def run_scans(kind, op, P, n, where, mode="plain"):
    """scan and scan_ltr, all P outputs guarded."""
    k, (out_off, in_offs) = KINDS[kind], place(P, where)
    ins = G.frozen(peer_inputs(kind, n, P), k.dtype, in_offs)
    tag = f"{mode} {kind} {op} P={P} n={n} {where}"
    for family, alg in SCANS:
        want = expected(mode, kind, op, family, n, P)
        into_guarded(k, want, n, out_off,
                     lambda bs: fmi_amd.scan_peers(OPS[op], alg, bs, ins.bs, accumulate_f32=(mode == "acc")),
                     op, f"{family} {tag}", count=P)
    ins.assert_intact(f"scans {tag}")


def ops_at(P):
    return ("sum", "prod", "max", "min") if P in (3, FUSED) else ("sum", "max")


def kinds_at(P):
    return ("f32", "i64", "f16", "bf16") + (("f64", "i32") if P <= FUSED else ())


# ---- the harness on the device: both calls are in bounds ----------------------------------------------------------------
def test_harness_reports_an_unwritten_element_and_a_written_guard(device):
    k, P, n = KINDS["f32"], 3, 516 * 4 - 1
    xs = peer_inputs("f32", n, P)
    want = expected("plain", "f32", "sum", "allreduce", n, P)[0]
    ins = G.frozen([x[:n - 1] for x in xs], k.dtype)
    (g,) = G.guarded_runs(want, n, k.dtype)
    fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, g.b.view(0, n - 1), ins.bs)  # n - 1 elements into a body of n
    fmi_amd.sync()
    with pytest.raises(AssertionError, match=f"element {n - 1} unwritten: 1 of {n}"):
        g.read(want, "one element short")
    assert not G.occurs(G.GUARD_BYTE, want, k.dtype)
    g = G.Guarded(n, k.dtype, poison=G.GUARD_BYTE)  # the body holds the guard byte, so a guard may be declared inside it
    g.read(None, "before the launch", declared_n=n - 2)
    fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, g.b.view(0, n - 1), ins.bs)
    fmi_amd.sync()
    got = g.read(want[:n - 1], "declared right", declared_n=n - 1)
    assert_bit_equal(got, want[:n - 1])
    assert 0xE7 not in want[n - 2:n - 1].view(np.uint8), "the last stored element must differ from the guard in every byte"
    with pytest.raises(AssertionError, match=r"guard written: 4 guard byte\(s\) changed, first at body \+ %d " % (4 * (n - 2))):
        g.read(want[:n - 2], "guard declared one element early", declared_n=n - 2)
    ins.assert_intact("harness")


def test_harness_holds_packed_fp4_buckets(device):
    """Guarded and frozen F4E2M1 buckets: n elements in (n + 1) // 2 bytes, judged byte by byte, an odd bucket's last high
    nibble 0. (The MXFP4 calls themselves are guarded in tests/test_gpu_mxfp4.py.)"""
    from tests import _mxfp4 as M

    n = 77
    xs, es = M.random_inputs(n, 1, 5)
    q, sc = G.FrozenSet([M.pack(xs[0])], DType.F4E2M1, 0, n=n), G.frozen([es[0]], DType.F8E8M0, 1)
    assert q.bs[0].nbytes == 39 and q.bs[0].n == n
    v = M.dequant(xs[0], es[0])
    for got in G.launched(v, n, DType.F32, lambda b: fmi_amd.mx_dequantize(b, q.bs[0], sc.bs[0]), "fp4 -> f32"):
        M.assert_mx(got, None, v, None, "f32", "fp4 -> f32")
    want, want_sc = M.quant(v)
    packed, wide = M.pack(want), G.frozen([v], DType.F32)
    for g, gs in mx_runs(packed, n, DType.F4E2M1, 0, want_sc):
        fmi_amd.mx_quantize(g.b, gs.b, wide.bs[0])
        fmi_amd.sync()
        got = g.read(packed, "f32 -> fp4")
        assert got.size == 39 and got[-1] >> 4 == 0
        M.assert_mx(M.unpack(got, n), gs.read(want_sc, "scales of f32 -> fp4"), want, want_sc, "same", "f32 -> fp4")
    for z in (q, sc, wide):
        z.assert_intact("fp4")


# ---- pairwise ------------------------------------------------------------------------------------------------------------
def pair_want(k, op, a, b):
    with np.errstate(all="ignore"):
        return k.f(op)(a, b)


@pytest.mark.parametrize("kind", list(KINDS))
def test_pairwise(device, kind):
    """reduce_pair (inout guarded, `in` frozen), combine (out guarded and poisoned, both operands frozen) and
    reduce_pair_batch (every size in one batch), all four ops; aligned, the written bucket off by one element, `in`
    off by one element."""
    k = KINDS[kind]
    for op in OPS:
        for where in PLACES:
            out_off, in_off = place(2, where)[0], place(2, where)[1][1]
            batch = []
            for n in k.sizes():
                a, b = peer_inputs(kind, n, 2)
                want, tag = pair_want(k, op, a, b), f"{kind} {op} n={n} {where}"
                src = G.frozen([b], k.dtype, in_off)
                g = G.Guarded(n, k.dtype, out_off).load([a])
                fmi_amd.reduce_pair(OPS[op], g.b, src.bs[0])
                fmi_amd.sync()
                k.same(g.read(None, f"reduce_pair {tag}"), want, op, f"reduce_pair {tag}")
                both = G.frozen([a, b], k.dtype, [0, in_off])
                into_guarded(k, want, n, out_off, lambda bs: fmi_amd.combine(OPS[op], bs[0], *both.bs), op, f"combine {tag}")
                both.assert_intact(f"combine {tag}")
                src.assert_intact(f"reduce_pair {tag}")
                batch.append((G.Guarded(n, k.dtype, out_off).load([a]), G.frozen([b], k.dtype, in_off), want, tag))
            fmi_amd.reduce_pair_batch(OPS[op], [(g.b, s.bs[0]) for g, s, _, _ in batch])
            fmi_amd.sync()
            for g, s, want, tag in batch:
                k.same(g.read(None, f"reduce_pair_batch {tag}"), want, op, f"reduce_pair_batch {tag}")
                s.assert_intact(f"reduce_pair_batch {tag}")


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_pairwise_every_launch_variant(device, variant):
    """FMI_TUNE_PAIR_VARIANT 0..4 at unroll 4, 256 threads: f32 and i8, the 515-group size and 16 tiles with a tail."""
    keys = (Tune.PAIR_VARIANT, Tune.PAIR_UNROLL, Tune.BLOCK)
    old = {key: fmi_amd.tune_get(key) for key in keys}
    try:
        for key, v in zip(keys, (variant, 4, 256)):
            fmi_amd.tune_set(key, v)
        for kind in ("f32", "i8"):
            k = KINDS[kind]
            for n in (516 * k.W - 1, 16 * 4 * 256 * k.W + k.W + 1):
                for where in PLACES:
                    out_off, in_off = place(2, where)[0], place(2, where)[1][1]
                    a, b = peer_inputs(kind, n, 2)
                    want, tag = pair_want(k, "sum", a, b), f"variant {variant} {kind} n={n} {where}"
                    src = G.frozen([b], k.dtype, in_off)
                    g = G.Guarded(n, k.dtype, out_off).load([a])
                    fmi_amd.reduce_pair(Op.SUM, g.b, src.bs[0])
                    fmi_amd.sync()
                    k.same(g.read(None, tag), want, "sum", tag)
                    both = G.frozen([a, b], k.dtype, [0, in_off])
                    into_guarded(k, want, n, out_off, lambda bs: fmi_amd.combine(Op.SUM, bs[0], *both.bs), "sum", f"combine {tag}")
                    both.assert_intact(tag)
                    src.assert_intact(tag)
    finally:
        for key, v in old.items():
            fmi_amd.tune_set(key, v)


# ---- the P-way programs ------------------------------------------------------------------------------------------------
PROGRAM_CASES = [(kind, P) for P in PEERS for kind in kinds_at(P)]  # f64 and i32 at the fused peer counts


@pytest.mark.parametrize("kind,P", PROGRAM_CASES)
def test_reduce_tree(device, kind, P):
    for op in ops_at(P):
        for n in KINDS[kind].sizes(P):
            for where in PLACES:
                run_trees(kind, op, P, n, where)


@pytest.mark.parametrize("kind,P", PROGRAM_CASES)
def test_scan_peers(device, kind, P):
    for op in ops_at(P):
        for n in KINDS[kind].sizes(P):
            for where in PLACES:
                run_scans(kind, op, P, n, where)


@pytest.mark.parametrize("P", [3, FUSED])
@pytest.mark.parametrize("policy", [0, 2], ids=["global_nt", "buffer_sc1"])
def test_fused_policy(device, policy, P):
    """FMI_TUNE_FUSED_POLICY at the values the policy tests use: every size, aligned (where the fused kernels run)."""
    old = fmi_amd.tune_get(Tune.FUSED_POLICY)
    try:
        fmi_amd.tune_set(Tune.FUSED_POLICY, policy)
        for kind in ("f32", "i64", "f16", "bf16"):
            for op in ("sum", "max"):
                for n in KINDS[kind].sizes(P):
                    run_trees(kind, op, P, n, "aligned")
                    run_scans(kind, op, P, n, "aligned")
    finally:
        fmi_amd.tune_set(Tune.FUSED_POLICY, old)


@pytest.mark.parametrize("P", [FUSED + 1, PREFOLD + 1, 3 * FUSED, ONE_PASS + 1, SCAN_ONE_PASS + 1])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_block_launches(device, kind, P):
    """FMI_TUNE_BLOCKS_ONE_PASS = 0: the blocked launches over the scratch arena's temporaries in place of the one-pass
    kernels (the matrix above runs the default, one pass)."""
    old = fmi_amd.tune_get(Tune.BLOCKS_ONE_PASS)
    try:
        fmi_amd.tune_set(Tune.BLOCKS_ONE_PASS, 0)
        for op in ("sum", "max"):
            for n in KINDS[kind].sizes(P):
                for where in ("aligned", "out+1"):
                    run_trees(kind, op, P, n, where)
                    run_scans(kind, op, P, n, where)
    finally:
        fmi_amd.tune_set(Tune.BLOCKS_ONE_PASS, old)


@pytest.mark.parametrize("P", [2, FUSED, FUSED + 1, PREFOLD + 1])
@pytest.mark.parametrize("kind", ["f16", "bf16", "e4m3", "e5m2"])
def test_acc_f32(device, kind, P):
    """FMI_ACC_F32: the fused kernels (2, 16) and the widen / f32 program / narrow fallback with its temporaries (17, 33,
    and every unaligned case)."""
    for op in ("sum", "prod"):
        for n in KINDS[kind].sizes(P):
            for where in ("aligned", "out+1"):
                run_trees(kind, op, P, n, where, "acc")
                run_scans(kind, op, P, n, where, "acc")


@pytest.mark.parametrize("P", [1, 3, FUSED, FUSED + 1])
@pytest.mark.parametrize("kind,mode", [("f32", "avg"), ("f64", "avg"), ("f16", "avg"), ("bf16", "avg"), ("f16", "avg_acc"),
                                       ("bf16", "avg_acc")])
def test_avg(device, kind, mode, P):
    for n in KINDS[kind].sizes(P):
        for where in ("aligned", "out+1"):
            run_trees(kind, "avg", P, n, where, mode)


@pytest.mark.parametrize("kind", ["f32", "f64", "f16", "bf16"])
def test_mean_scale_alone(device, kind):
    """fmi_dev_mean_scale in place on a guarded bucket, aligned and one element off."""
    k = KINDS[kind]
    for n in k.sizes():
        for off in (0, 1):
            for P in (3, 7):
                x = AV.inputs(kind, n, 71, 0)
                S = H.widen(x, kind) if AV.is_half(kind) else x
                g = G.Guarded(n, k.dtype, off).load([x])
                fmi_amd.mean_scale(g.b, P)
                fmi_amd.sync()
                tag = f"mean_scale {kind} n={n} P={P} offset {off}"
                AV.assert_same(k.bits(g.read(None, tag)), AV.scale(S, kind, P), kind, tag)


@pytest.mark.parametrize("P", [3, FUSED + 1])
@pytest.mark.parametrize("kind", ["e4m3", "e5m2"])
def test_fp8_plain_programs(device, kind, P):
    """The plain FP8 P-way programs: pairwise passes in the program's order."""
    for op in ("sum", "max"):
        for n in KINDS[kind].sizes(P):
            for where in ("aligned", "out+1"):
                run_trees(kind, op, P, n, where)
                run_scans(kind, op, P, n, where)


# ---- the scaled FP8 reductions -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 8, FUSED, FUSED + 1])
@pytest.mark.parametrize("out", ["same", "f32"])
@pytest.mark.parametrize("kind", ["e4m3", "e5m2"])
def test_reduce_tree_scaled(device, kind, out, P):
    """The one-float amax slot sits alone inside a guarded region, off 16-B alignment; the scale arrays are frozen."""
    k, s = KINDS[kind], FS.scales(P)
    ko = k if out == "same" else KINDS["f32"]
    for n in k.sizes(P):
        for off in (0, 1):
            ins = G.frozen(peer_inputs(kind, n, P), k.dtype, off)
            scales, t = G.frozen([s], DType.F32), G.frozen([np.array([FS.T_OUT], np.float32)], DType.F32, 3)
            for family, alg, root in (("allreduce", Alg.ALLREDUCE, 0), ("reduce", Alg.REDUCE, P - 1), ("reduce_ltr", Alg.REDUCE_LTR, 0)):
                want, want_amax, _ = FS.expected_scaled(family, kind, list(peer_inputs(kind, n, P)), s, FS.T_OUT, out, root)
                tag = f"scaled {kind} {family} P={P} n={n} out={out} offset {off}"
                for g in G.guarded_runs(want, n, ko.dtype, off):
                    am = G.Guarded(1, DType.F32, 7).load([np.zeros(1, np.float32)])
                    fmi_amd.reduce_tree_scaled(alg, g.b, ins.bs, scales.bs[0], t.bs[0], am.b, rank=root)
                    fmi_amd.sync()
                    FS.assert_out(g.read(want, tag), want, kind, out, tag)
                    FS.assert_amax(int(am.read(None, f"amax of {tag}").view(np.uint32)[0]), want_amax, tag)
            for z in (ins, scales, t):
                z.assert_intact(f"scaled {kind} P={P} n={n} out={out} offset {off}")


# ---- block-scaled FP8 (tests/test_gpu_mx.py pre-fills its outputs but keeps no guards; MXFP4 is guarded in
# tests/test_gpu_mxfp4.py::Out) -----------------------------------------------------------------------------------------------
def mx_runs(want, n, dtype, off, want_sc):
    """(elements, scale bytes) outputs for one MX call, the scale bytes at an odd address (None for an f32 result): as
    many runs as the longer of the two poison choices needs, the other output poisoned again for its second run."""
    runs = G.guarded_runs(want, n, dtype, off)
    sruns = [None] if want_sc is None else G.guarded_runs(want_sc, MX.blocks(n), DType.F8E8M0, 1)
    for j in range(max(len(runs), len(sruns))):
        g, gs = runs[j % len(runs)], sruns[j % len(sruns)]
        if j >= len(runs):
            g.repoison()
        if j >= len(sruns) and gs is not None:
            gs.repoison()
        yield g, gs


@pytest.mark.parametrize("src", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("kind", ["e4m3", "e5m2"])
def test_mx_quantize_dequantize(device, kind, src):
    """mx_dequantize into a guarded f32 / f16 / bf16 bucket and mx_quantize from it into guarded elements and scale
    bytes; aligned and one element off."""
    k, ks = KINDS[kind], KINDS[src]
    for n in (1, 31, 32, 33, 516 * 16 - 1):
        xs, es = MX.random_inputs(kind, n, 1, 7, finite=True)
        v = MX.dequant(xs[0], es[0], kind)
        wide = v if src == "f32" else H.narrow(v, src)
        want, want_sc = MX.quant(to_f32(wide, src), kind)
        for off in (0, 1):
            q, e = G.frozen(xs, k.dtype, off), G.frozen(es, DType.F8E8M0, 1)
            tag = f"mx {kind} <-> {src} n={n} offset {off}"
            into_guarded(ks, wide, n, off, lambda bs: fmi_amd.mx_dequantize(bs[0], q.bs[0], e.bs[0]), "sum", f"dequantize {tag}")
            q.assert_intact(tag)
            e.assert_intact(tag)
            w = G.frozen([wide], ks.dtype, off)
            for g, gs in mx_runs(want, n, k.dtype, off, want_sc):
                fmi_amd.mx_quantize(g.b, gs.b, w.bs[0])
                fmi_amd.sync()
                MX.assert_mx(g.read(want, f"quantize {tag}"), gs.read(want_sc, f"scales of quantize {tag}"), want, want_sc, kind,
                             "same", f"quantize {tag}")
            w.assert_intact(tag)


@pytest.mark.parametrize("P", [2, FUSED, FUSED + 1])
@pytest.mark.parametrize("kind", ["e4m3", "e5m2"])
def test_reduce_tree_mx(device, kind, P):
    """Elements and scale bytes guarded, the scale bytes at an odd address; inputs and their scales frozen."""
    k = KINDS[kind]
    for n in (1, 31, 33, 516 * 16 - 1):
        xs, es = MX.random_inputs(kind, n, P, 7)
        for out in ("same", "f32"):
            for off in (0, 1):
                ins, scs = G.frozen(xs, k.dtype, off), G.frozen(es, DType.F8E8M0, 1)
                for family, alg, root in (("allreduce", Alg.ALLREDUCE, 0), ("reduce", Alg.REDUCE, P - 1), ("reduce_ltr", Alg.REDUCE_LTR, 0)):
                    want, want_sc = MX.expected_mx(family, kind, xs, es, "sum", out, root)
                    tag = f"mx {kind} {family} P={P} n={n} out={out} offset {off}"
                    for g, gs in mx_runs(want, n, k.dtype if out == "same" else DType.F32, off if out == "same" else 0, want_sc):
                        fmi_amd.reduce_tree_mx(Op.SUM, alg, g.b, None if gs is None else gs.b, ins.bs, scs.bs, rank=root)
                        fmi_amd.sync()
                        got = g.read(want, tag)
                        got_sc = None if gs is None else gs.read(want_sc, f"scales of {tag}")
                        MX.assert_mx(got.view(np.float32) if out == "f32" else got, got_sc, want, want_sc, kind, out, tag)
                ins.assert_intact(f"mx {kind} P={P} n={n} out={out} offset {off}")
                scs.assert_intact(f"mx scales {kind} P={P} n={n} out={out} offset {off}")


# ---- conversions, fills, copies ------------------------------------------------------------------------------------------
FLOATS = ("f32", "f16", "bf16", "e4m3", "e5m2")


def to_f32(bits, kind):
    return np.asarray(bits, np.float32) if kind == "f32" else H.widen(bits, kind) if kind in H.KINDS else F.widen(bits, kind)


def from_f32(x, kind):
    return np.asarray(x, np.float32) if kind == "f32" else H.narrow(x, kind) if kind in H.KINDS else F.narrow(x, kind)


@functools.lru_cache(maxsize=None)
def convert_source(kind, n):
    """n values of `kind` spread over its whole range: every 8-bit pattern, 16-bit patterns in steps of 31, and for f32
    the boundary set of tests/_fp8.py in steps of 47."""
    i = np.arange(n, dtype=np.uint64)
    if kind == "f32":
        b = F.boundary_f32()
        return b[(i * np.uint64(47)) % np.uint64(b.size)].copy()
    if kind in H.KINDS:
        return ((i * np.uint64(31)) % np.uint64(65536)).astype(np.uint16)
    return (i % np.uint64(256)).astype(np.uint8)


@pytest.mark.parametrize("dst", FLOATS)
@pytest.mark.parametrize("src", FLOATS)
def test_convert(device, src, dst):
    ks, kd = KINDS[src], KINDS[dst]
    W = 16 // min(ks.size, kd.size)
    for n in (1, W - 1, W, W + 1, 516 * W - 1):
        x = convert_source(src, n)
        with np.errstate(all="ignore"):
            want = from_f32(to_f32(x, src), dst)
        for off in (0, 1):
            s = G.frozen([x], ks.dtype)
            tag = f"convert {src} -> {dst} n={n} dst offset {off}"
            into_guarded(kd, want, n, off, lambda bs: fmi_amd.convert(bs[0], s.bs[0]), "sum", tag)
            s.assert_intact(tag)


@pytest.mark.parametrize("kind", list(KINDS))
def test_fill_synthetic(device, kind):
    k = KINDS[kind]
    for n in k.sizes():
        for off in (0, 1):
            for peer in (0, 5):
                want = (H.synthetic(kind, n, 42, peer) if kind in H.KINDS else F.synthetic(kind, n, 42, peer) if kind in F.KINDS
                        else orc.synthetic(k.np, n, seed=42, peer=peer))
                into_guarded(k, want, n, off, lambda bs: bs[0].fill_synthetic(42, peer), "max", f"fill_synthetic {kind} n={n} offset {off}")


@pytest.mark.parametrize("nbytes", [16, 262143, 262144 + 5])
def test_device_copy(device, nbytes):
    """fmi_dev_d2d_async below and at the copy kernel's threshold, with its sub-16-B tail; aligned and unaligned."""
    k = KINDS["u8"]
    data = np.random.default_rng(nbytes).integers(0, 256, nbytes, dtype=np.uint8)
    for dst_off, src_off in ((0, 0), (3, 0), (0, 1)):
        src = G.frozen([data], k.dtype, src_off)
        tag = f"d2d {nbytes} bytes, offsets {dst_off}/{src_off}"
        into_guarded(k, data, nbytes, dst_off, lambda bs: bs[0].copy_from(src.bs[0]), "max", tag)
        src.assert_intact(tag)


def test_memset_async(device):
    k = KINDS["u8"]
    for nbytes in (1, 15, 16, 17, 516 * 16 - 1, 262144 + 5):
        for off in (0, 1):
            for value in (0x00, 0x5A):
                into_guarded(k, np.full(nbytes, value, np.uint8), nbytes, off,
                             lambda bs: fmi_amd._lib.call("fmi_dev_memset_async", bs[0].ptr, value, nbytes, None), "max",
                             f"memset {nbytes} bytes of 0x{value:02x}, offset {off}")


# ---- the communicator: LOCAL transport, every rank's recv guarded --------------------------------------------------------
def comm_case(N, k, wants, sends, call, what, op="sum"):
    """Every rank r runs `call(c, r, send bucket, recv bucket or None)` with its `send` frozen and its recv guarded
    (ranks whose wants[r] is None have no recv). One poison choice for all ranks, so every rank makes the same calls."""
    from tests.test_gpu_comm import run_ranks

    have = [w for w in wants if w is not None]
    poisons = G.poisons_for(have, k.dtype)

    def body(c, r):
        s = None if sends[r] is None else G.frozen([sends[r]], k.dtype)
        gs = []
        for p in poisons:
            g = None if wants[r] is None else G.Guarded(np.asarray(wants[r]).size, k.dtype, 0, p, paired=len(poisons) == 2)
            call(c, r, None if s is None else s.bs[0], None if g is None else g.b)
            gs.append(g)
        fmi_amd.sync()
        return s, gs

    # judged here, after every rank has returned: a rank that stopped early would leave the others waiting for it
    res = run_ranks(N, body)
    fmi_amd.sync()
    for r, (s, gs) in enumerate(res):
        for g in gs:
            if g is not None:
                k.same(g.read(wants[r], f"{what} rank {r}"), wants[r], op, f"{what} rank {r}")
        if s is not None:
            s.assert_intact(f"{what} rank {r}")


@pytest.mark.parametrize("N", [2, 3])
def test_comm_reductions(device, N):
    k = KINDS["f32"]
    n = 516 * 4 - 1  # 2063: divisible by neither 2 nor 3
    xs = [core_inputs(np.float32, n, r, seed=11) for r in range(N)]
    with np.errstate(all="ignore"):
        for op in ("sum", "max"):
            f = orc.OPS[op]
            comm_case(N, k, orc.allreduce(xs, f)[0], xs, lambda c, r, s, o: c.allreduce(OPS[op], s, o), f"allreduce {op} N={N}", op)
            comm_case(N, k, orc.allreduce(xs, f, commutative=False, associative=False)[0], xs,
                      lambda c, r, s, o: c.allreduce(OPS[op], s, o, ordered=True), f"allreduce ordered {op} N={N}", op)
            for ordered in (False, True):
                comm_case(N, k, orc.scan(xs, f, commutative=not ordered, associative=not ordered)[0], xs,
                          lambda c, r, s, o: c.scan(OPS[op], s, o, ordered=ordered), f"scan ordered={ordered} {op} N={N}", op)
                for root in (0, N - 1):
                    want = orc.reduce(xs, f, root=root, commutative=not ordered, associative=not ordered)[0]
                    comm_case(N, k, [want if r == root else None for r in range(N)], xs,
                              lambda c, r, s, o: c.reduce(OPS[op], s, o, root, ordered=ordered),
                              f"reduce root {root} ordered={ordered} {op} N={N}", op)


@pytest.mark.parametrize("N", [2, 3])
def test_comm_data_movement(device, N):
    k, n = KINDS["i64"], 516 * 2 + 1
    xs = [core_inputs(np.int64, n, r, seed=13) for r in range(N)]
    whole = np.concatenate(xs)
    for root in (0, N - 1):
        comm_case(N, k, [whole if r == root else None for r in range(N)], xs, lambda c, r, s, o: c.gather(s, o, root),
                  f"gather root {root} N={N}", "max")
        comm_case(N, k, xs, [whole if r == root else None for r in range(N)], lambda c, r, s, o: c.scatter(s, o, root),
                  f"scatter root {root} N={N}", "max")
        # bcast: the root's buffer is an input, everyone else's an output
        comm_case(N, k, [None if r == root else xs[root] for r in range(N)], [xs[root] if r == root else None for r in range(N)],
                  lambda c, r, s, o: c.bcast(s if r == root else o, root), f"bcast root {root} N={N}", "max")


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("kind", ["e4m3", "e5m2"])
def test_comm_allreduce_scaled(device, kind, N):
    from tests.test_gpu_comm import run_ranks

    k, n = KINDS[kind], 516 * 16 - 1
    xs, s = [F.synthetic(kind, n, 81, r) for r in range(N)], FS.scales(N)
    for out in ("same", "f32"):
        ko = k if out == "same" else KINDS["f32"]
        for ordered in (False, True):
            want, want_amax, _ = FS.expected_scaled("allreduce_ltr" if ordered else "allreduce", kind, xs, s, FS.T_OUT, out)
            poisons = G.poisons_for(want, ko.dtype)
            tag = f"allreduce_scaled {kind} N={N} out={out} ordered={ordered}"

            def body(c, r):
                send = G.frozen([xs[r]], k.dtype)
                scale, t = G.frozen([s[r:r + 1]], DType.F32, 1), G.frozen([np.array([FS.T_OUT], np.float32)], DType.F32, 2)
                outs = []
                for p in poisons:
                    g = G.Guarded(n, ko.dtype, 0, p, paired=len(poisons) == 2)
                    am = G.Guarded(1, DType.F32, 7).load([np.zeros(1, np.float32)])
                    c.allreduce_scaled(send.bs[0], scale.bs[0], g.b, t.bs[0], am.b, ordered=ordered)
                    outs.append((g, am))
                fmi_amd.sync()
                return (send, scale, t), outs

            res = run_ranks(N, body)  # judged after every rank has returned
            fmi_amd.sync()
            for r, (ins, outs) in enumerate(res):
                for g, am in outs:
                    FS.assert_out(g.read(want, f"{tag} rank {r}"), want, kind, out, f"{tag} rank {r}")
                    FS.assert_amax(int(am.read(None, f"amax of {tag} rank {r}").view(np.uint32)[0]), want_amax, f"{tag} rank {r}")
                for z in ins:
                    z.assert_intact(f"{tag} rank {r}")


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("kind", ["e4m3", "e5m2"])
def test_comm_allreduce_mx(device, kind, N):
    """MXFP8 (tests/test_gpu_mxfp4.py::test_comm_allreduce_mx guards MXFP4's): recv and its scale bytes guarded, send and its
    scale bytes frozen; n divisible by neither the rank count nor the block."""
    from tests.test_gpu_comm import run_ranks

    k, n = KINDS[kind], 516 * 16 - 1
    xs, es = MX.random_inputs(kind, n, N, seed=81, finite=True)
    for out in ("same", "f32"):
        for ordered in (False, True):
            want, want_sc = MX.expected_mx("allreduce_ltr" if ordered else "allreduce", kind, xs, es, "sum", out)
            tag = f"allreduce_mx {kind} N={N} out={out} ordered={ordered}"
            # the same number of calls on every rank: the poisons are chosen here, from what every rank expects
            poisons = G.poisons_for(want, k.dtype if out == "same" else DType.F32)
            spoisons = [None] if out == "f32" else G.poisons_for(want_sc, DType.F8E8M0)
            runs = max(len(poisons), len(spoisons))

            def body(c, r):
                send, ssc, outs = G.frozen([xs[r]], k.dtype), G.frozen([es[r]], DType.F8E8M0, 1), []
                for j in range(runs):
                    g = G.Guarded(n, k.dtype if out == "same" else DType.F32, 0, poisons[j % len(poisons)], paired=len(poisons) == 2)
                    gs = None if out == "f32" else G.Guarded(MX.blocks(n), DType.F8E8M0, 1, spoisons[j % len(spoisons)],
                                                               paired=len(spoisons) == 2)
                    c.allreduce_mx(Op.SUM, send.bs[0], ssc.bs[0], g.b, None if gs is None else gs.b, ordered=ordered)
                    outs.append((g, gs))
                fmi_amd.sync()
                return (send, ssc), outs

            res = run_ranks(N, body)  # judged after every rank has returned
            fmi_amd.sync()
            for r, (ins, outs) in enumerate(res):
                for g, gs in outs:
                    got = g.read(want, f"{tag} rank {r}")
                    got_sc = None if gs is None else gs.read(want_sc, f"scales of {tag} rank {r}")
                    MX.assert_mx(got, got_sc, want, want_sc, kind, out, f"{tag} rank {r}")
                for z in ins:
                    z.assert_intact(f"{tag} rank {r}")
