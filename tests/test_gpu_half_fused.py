"""FMI_F16 / FMI_BF16 buckets through every fused and one-pass P-way family on the MI355X: the left-to-right forms,
reduce partials, 17..31 peers, the one-pass chains, blocked trees, pre-fold allreduces and blocked scans, the
communicator's ordered and wide collectives, and graph capture. Every comparison is on the 16 raw bits against
tests/_half.py's combine driven through oracle.fmi_oracle's event-driven simulation (tests/test_gpu_half.py's
helpers and edge sprinkling), so the expected values are the reference's order at every P
(tests/test_half_fused_cpu.py pins the programs to it)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import fmi_amd
from fmi_amd import Alg, Bucket, Graph, Op, Stream, Tune
from fmi_amd.comm import Path
from oracle import fmi_oracle as orc
from tests import _guard as G
from tests import _half as H
from tests._half_fused_cases import (ALLREDUCE_P, LTR_P, REDUCE_P, SCAN_P, allreduce_ranks, extra_ops_at, reduce_roots)
from tests.test_gpu_half import DT, FUSED_SIZES, OP, bucket, read

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_SIZES = [7, 2061]  # 2061: one 256-thread tile of 8-lane vectors + one vector + a 5-element tail


def sizes(P):
    return FUSED_SIZES if P <= 16 else WIDE_SIZES


def ops_at(family, P):
    return ("sum", "max") + (("prod", "min") if P == extra_ops_at[family] else ())


@functools.lru_cache(maxsize=None)
def peer_bits(kind, n, P, seed):
    xs = tuple(H.inputs(kind, n, seed=seed, peer=p) for p in range(P))
    for x in xs:
        x.setflags(write=False)
    return xs


@functools.lru_cache(maxsize=None)
def expected(family, kind, op, n, P, seed, root=0):
    """The oracle's value(s), computed once per case and left unchanged: a list per rank for allreduce / scan /
    scan_ltr, (result, sendbufs) for reduce, one array for reduce_ltr."""
    xs, f = list(peer_bits(kind, n, P, seed)), H.combiner(op, kind)
    if family == "allreduce":
        return orc.allreduce(xs, f)[0]
    if family == "allreduce_ltr":
        return orc.allreduce(xs, f, commutative=False, associative=False)[0]
    if family == "reduce":
        return orc.reduce(xs, f, root=root)
    if family == "reduce_ltr":
        return orc.reduce(xs, f, root=0, commutative=False, associative=False)[0]
    if family == "scan":
        return orc.scan(xs, f)[0]
    if family == "scan_ltr":
        return orc.scan(xs, f, commutative=False, associative=False)[0]
    raise ValueError(family)


def upload(kind, n, P, seed):
    return [bucket(x, kind) for x in peer_bits(kind, n, P, seed)]


def run_scan(alg, kind, op, n, P, seed, what, alias=False):
    """Outputs of their own are guarded and poisoned (tests/_guard.py); aliased ones are the inputs themselves."""
    ins = upload(kind, n, P, seed)
    want = expected("scan" if alg == Alg.SCAN else "scan_ltr", kind, op, n, P, seed)
    if alias:
        fmi_amd.scan_peers(OP[op], alg, ins, ins)
        fmi_amd.sync()
        gots = [[read(b) for b in ins]]
    else:
        gots = G.launched_all(want, n, DT[kind], lambda outs: fmi_amd.scan_peers(OP[op], alg, outs, ins),
                              f"{what} {kind} {op} P={P} n={n}")
    for got in gots:
        for r in range(P):
            H.assert_bits(got[r].view(np.uint16), want[r], kind, op, f"{what} {kind} {op} P={P} n={n} output {r}")


def run_tree(alg, kind, op, ins, want, what, rank=0):
    """One reduce_tree call into a guarded, poisoned output, compared on its 16 raw bits."""
    for got in G.launched(want, want.size, DT[kind], lambda out: fmi_amd.reduce_tree(OP[op], alg, out, ins, rank=rank), what):
        H.assert_bits(got.view(np.uint16), want, kind, op, what)


def run_allreduce(kind, op, n, P, seed, what):
    want = expected("allreduce", kind, op, n, P, seed)
    ins = upload(kind, n, P, seed)
    for r in allreduce_ranks(op, P):
        run_tree(Alg.ALLREDUCE, kind, op, ins, want[r], f"{what} {kind} {op} P={P} n={n} rank {r}", rank=r)
    if op == "max":  # ±0 ties: a kernel that hands every rank rank 0's bits fails above only if the ranks differ
        assert any(not np.array_equal(want[0], want[r]) for r in range(1, P)), "at least two ranks must differ on ±0"


@pytest.fixture(params=[0, 2], ids=["global_nt", "buffer_sc1"])
def fused_policy(request, device):
    """FMI_TUNE_FUSED_POLICY at the global and the buffer form, restored afterwards."""
    old = fmi_amd.tune_get(Tune.FUSED_POLICY)
    fmi_amd.tune_set(Tune.FUSED_POLICY, request.param)
    yield request.param
    fmi_amd.tune_set(Tune.FUSED_POLICY, old)


@pytest.fixture(params=[1, 0], ids=["one_pass", "block_launches"])
def blocks_one_pass(request, device):
    """FMI_TUNE_BLOCKS_ONE_PASS on and off, restored afterwards: off runs the blocked launches with arena temps."""
    old = fmi_amd.tune_get(Tune.BLOCKS_ONE_PASS)
    fmi_amd.tune_set(Tune.BLOCKS_ONE_PASS, request.param)
    yield request.param
    fmi_amd.tune_set(Tune.BLOCKS_ONE_PASS, old)


@pytest.mark.parametrize("P", LTR_P)
@pytest.mark.parametrize("kind", H.KINDS)
def test_reduce_ltr_and_scan_ltr(device, kind, P):
    """Fused up to 31 peers, the one-pass chain up to 128, segments with a carry-in beyond."""
    for op in ops_at("ltr", P):
        for n in sizes(P):
            run_tree(Alg.REDUCE_LTR, kind, op, upload(kind, n, P, seed=21), expected("reduce_ltr", kind, op, n, P, 21),
                     f"reduce_ltr {kind} {op} P={P} n={n}")
            run_scan(Alg.SCAN_LTR, kind, op, n, P, 21, "scan_ltr")


@pytest.mark.parametrize("kind", H.KINDS)
def test_scan_outputs_alias_inputs(device, kind):
    for alg, P in ((Alg.SCAN_LTR, 5), (Alg.SCAN_LTR, 33), (Alg.SCAN, 17)):
        run_scan(alg, kind, "sum", 2061, P, 22, "in-place scan", alias=True)


@pytest.mark.parametrize("P", REDUCE_P)
@pytest.mark.parametrize("kind", H.KINDS)
def test_reduce_wide_roots(device, kind, P):
    for op in ops_at("reduce", P):
        for n in sizes(P):
            ins = upload(kind, n, P, seed=23)
            for root in reduce_roots(P):
                run_tree(Alg.REDUCE, kind, op, ins, expected("reduce", kind, op, n, P, 23, root)[0],
                         f"reduce {kind} {op} P={P} n={n} root {root}", rank=root)


@pytest.mark.parametrize("P", ALLREDUCE_P)
@pytest.mark.parametrize("kind", H.KINDS)
def test_allreduce_wide_ranks(device, kind, P):
    for op in ops_at("allreduce", P):
        for n in sizes(P):
            run_allreduce(kind, op, n, P, 24, "allreduce")


@pytest.mark.parametrize("P", SCAN_P)
@pytest.mark.parametrize("kind", H.KINDS)
def test_scan_wide_every_output(device, kind, P):
    for op in ops_at("scan", P):
        for n in sizes(P):
            run_scan(Alg.SCAN, kind, op, n, P, 25, "scan")


@pytest.mark.parametrize("kind", H.KINDS)
def test_blocked_launches_and_one_pass(blocks_one_pass, kind):
    """P = 48 allreduce and P = 33 / 64 scan in both modes: the block launches run the fused carry programs, the
    32-input pre-fold block and the 16-peer reduce over arena temps. scan_ltr at P = 32: its block launches continue
    the chain from a carry over 15 peers and then over 1, the largest and the smallest program of the chain-carry
    unit (n = 4099: whole 16-B lane groups and a ragged tail); one pass is the chain kernel."""
    for op in ("sum", "max"):
        for n in WIDE_SIZES:
            run_allreduce(kind, op, n, 48, 24, f"allreduce one_pass={blocks_one_pass}")
            for P in (33, 64):
                run_scan(Alg.SCAN, kind, op, n, P, 25, f"scan one_pass={blocks_one_pass}")
        run_scan(Alg.SCAN_LTR, kind, op, 4099, 32, 21, f"scan_ltr one_pass={blocks_one_pass}")


@pytest.mark.parametrize("kind", H.KINDS)
def test_buffer_and_global_policy(fused_policy, kind):
    """One P per family of the kernels that take FMI_TUNE_FUSED_POLICY."""
    for op in ("sum", "max"):
        for n in WIDE_SIZES:
            run_tree(Alg.REDUCE_LTR, kind, op, upload(kind, n, 5, seed=21), expected("reduce_ltr", kind, op, n, 5, 21),
                     f"reduce_ltr P=5 n={n}")
            run_scan(Alg.SCAN_LTR, kind, op, n, 16, 21, "scan_ltr")
            run_allreduce(kind, op, n, 24, 24, "allreduce")
            run_scan(Alg.SCAN, kind, op, n, 31, 25, "scan")


@pytest.mark.parametrize("N", [3, 8])
@pytest.mark.parametrize("kind,op", [("bf16", "sum"), ("f16", "max")])
def test_comm_reduce_sendbuf_partials(device, N, kind, op):
    """fmi_comm_reduce_sendbuf (the fused reduce-partials kernel on every rank's shard): the root's recv and every
    rank's sendbuf as the reference leaves them."""
    from tests.test_gpu_comm import run_ranks

    n = 4 * 2048 + 5
    xs = peer_bits(kind, n, N, 26)
    for root in (0, N - 1):
        def body(c, r):
            s, out = bucket(xs[r], kind), Bucket(n, DT[kind])
            c.reduce(OP[op], s, out if r == root else None, root, sendbuf_partials=True)
            fmi_amd.sync()
            return read(s), read(out) if r == root else None

        res = run_ranks(N, body)
        want, sends = expected("reduce", kind, op, n, N, 26, root)
        H.assert_bits(res[root][1], want, kind, op, f"{kind} {op} N={N} root {root} result")
        for r in range(N):
            H.assert_bits(res[r][0], sends[r], kind, op, f"{kind} {op} N={N} root {root}: sendbuf of rank {r}")


@pytest.mark.parametrize("kind,op", [("bf16", "sum"), ("f16", "max")])
def test_comm_ordered_collectives(device, kind, op):
    """N = 4: allreduce with FMI_ALG_REDUCE_LTR and scan with FMI_ALG_SCAN_LTR."""
    from tests.test_gpu_comm import run_ranks

    N, n = 4, 4 * 2048 + 5
    xs = peer_bits(kind, n, N, 27)

    def body(c, r):
        s, out, sc = bucket(xs[r], kind), Bucket(n, DT[kind]), Bucket(n, DT[kind])
        c.allreduce(OP[op], s, out, ordered=True)
        c.scan(OP[op], s, sc, ordered=True)
        fmi_amd.sync()
        return read(out), read(sc)

    res = run_ranks(N, body)
    want_ar = expected("allreduce_ltr", kind, op, n, N, 27)
    want_sc = expected("scan_ltr", kind, op, n, N, 27)
    for r in range(N):
        H.assert_bits(res[r][0], want_ar[r], kind, op, f"ordered allreduce {kind} {op} rank {r}")
        H.assert_bits(res[r][1], want_sc[r], kind, op, f"ordered scan {kind} {op} rank {r}")


@pytest.mark.parametrize("kind,op", [("bf16", "sum"), ("f16", "max")])
def test_comm_allreduce_twenty_ranks(device, kind, op):
    """N = 20, path TREE: every rank's shard reduction is the fused 20-peer allreduce, per-rank bits for max."""
    from tests.test_gpu_comm import run_ranks

    N, n = 20, 4099
    xs = peer_bits(kind, n, N, 28)

    def body(c, r):
        s, out = bucket(xs[r], kind), Bucket(n, DT[kind])
        c.allreduce(OP[op], s, out, path=Path.TREE)
        fmi_amd.sync()
        return read(out)

    res = run_ranks(N, body)
    want = expected("allreduce", kind, op, n, N, 28)
    for r in range(N):
        H.assert_bits(res[r], want[r], kind, op, f"comm allreduce {kind} {op} N=20 rank {r}")
    if op == "max":
        assert any(not np.array_equal(want[0], want[r]) for r in range(1, N))


def test_graph_capture_ordered_and_wide(device):
    """REDUCE_LTR and SCAN_LTR at 5 peers, ALLREDUCE at 17 and REDUCE at 40 need no arena for bf16: they capture
    into a graph, and its replays follow re-uploaded inputs."""
    kind, op, n = "bf16", "sum", 2061
    st = Stream()
    ins5, ins17, ins40 = ([Bucket(n, DT[kind]) for _ in range(P)] for P in (5, 17, 40))
    ltr, ar, red = Bucket(n, DT[kind]), Bucket(n, DT[kind]), Bucket(n, DT[kind])
    scans = [Bucket(n, DT[kind]) for _ in range(5)]

    def record():
        fmi_amd.reduce_tree(Op.SUM, Alg.REDUCE_LTR, ltr, ins5, stream=st)
        fmi_amd.scan_peers(Op.SUM, Alg.SCAN_LTR, scans, ins5, stream=st)
        fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, ar, ins17, rank=16, stream=st)
        fmi_amd.reduce_tree(Op.SUM, Alg.REDUCE, red, ins40, rank=5, stream=st)

    g = Graph.capture(st, record)
    try:
        for seed in (31, 32):
            for ins in (ins5, ins17, ins40):
                for b, x in zip(ins, peer_bits(kind, n, len(ins), seed)):
                    b.upload(x)
            g.launch(st)
            st.sync()
            H.assert_bits(read(ltr), expected("reduce_ltr", kind, op, n, 5, seed), kind, op, f"replay {seed}: reduce_ltr")
            want = expected("scan_ltr", kind, op, n, 5, seed)
            for r in range(5):
                H.assert_bits(read(scans[r]), want[r], kind, op, f"replay {seed}: scan_ltr output {r}")
            H.assert_bits(read(ar), expected("allreduce", kind, op, n, 17, seed)[16], kind, op, f"replay {seed}: allreduce")
            H.assert_bits(read(red), expected("reduce", kind, op, n, 40, seed, 5)[0], kind, op, f"replay {seed}: reduce")
    finally:
        g.destroy()
        st.destroy()


def test_unaligned_stays_stepwise(device):
    """A 2-byte-offset view has no fused kernel: the same bits through pairwise passes, and, needing the arena,
    still refused under capture."""
    kind, op, n, P = "bf16", "sum", 2061, 5
    xs = peer_bits(kind, n, P, 33)
    padded = [np.concatenate([np.zeros(1, np.uint16), x]) for x in xs]
    ins = [bucket(x, kind).view(1, n) for x in padded]
    out = Bucket(n, DT[kind])
    fmi_amd.reduce_tree(Op.SUM, Alg.REDUCE_LTR, out, ins)
    fmi_amd.sync()
    H.assert_bits(read(out), expected("reduce_ltr", kind, op, n, P, 33), kind, op, "unaligned reduce_ltr P=5")
    st = Stream()
    try:
        with pytest.raises(fmi_amd.FmiError, match="FMI_ERR_UNSUPPORTED.*graph"):
            Graph.capture(st, lambda: fmi_amd.reduce_tree(Op.SUM, Alg.REDUCE_LTR, out, ins, stream=st))
    finally:
        st.destroy()


def test_cpp_half_ordered_gpu(device):
    """Data<Dev::Bucket<Dev::bfloat16>> through FMI::Communicator::allreduce and scan with a non-commutative
    Function (reduce_ltr / scan_ltr), 3 peers: equal to the program's own host-path results bit for bit
    (fmi_amd/cpp/tests/test_half_ordered.cpp)."""
    exe = os.path.join(ROOT, "build", "cpp", "test_half_ordered")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fmi_amd", "cpp")], check=True)
    out = subprocess.run([exe, "--gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    assert "0 failed checks" in out.stderr
