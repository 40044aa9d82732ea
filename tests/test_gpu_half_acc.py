"""FMI_ACC_F32 on the MI355X: FMI_F16 / FMI_BF16 buckets reduced with the program's values kept in f32 and every
stored output rounded once. The fused kernels (2..16 peers, aligned), the fallback (widen, the FMI_F32 program,
narrow) beyond them, both cache policies, every 16-bit pattern, the communicator's shard steps and graph capture.
Every comparison is on the 16 raw bits against tests/_half_acc.py: oracle.fmi_oracle's event-driven simulation over
the widened f32 arrays with an np.float32 op, narrowed once per stored output."""
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
from tests import _half_acc as A
from tests.test_gpu_half import DT, OP, bucket, read

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [7, 2061, 4 * 2048 + 5]  # 2061: one 256-thread tile of 8-lane groups + one group + a 5-element tail
WIDE_SIZES = [7, 2061]
FUSED_P = [2, 3, 5, 8, 13, 16]


@functools.lru_cache(maxsize=None)
def peer_bits(src, kind, n, P, seed):
    """src "inputs": the synthetic fill with the edge values sprinkled in; "cancel": A.cancel_inputs."""
    xs = A.cancel_inputs(kind, n, P, seed) if src == "cancel" else [H.inputs(kind, n, seed=seed, peer=p) for p in range(P)]
    for x in xs:
        x.setflags(write=False)
    return tuple(xs)


@functools.lru_cache(maxsize=None)
def want(family, src, kind, op, n, P, seed, root=0):
    """The oracle's value(s), computed once per case and left unchanged (A.expected_acc's shapes)."""
    return A.expected_acc(family, kind, op, list(peer_bits(src, kind, n, P, seed)), root)


def upload(src, kind, n, P, seed):
    return [bucket(x, kind) for x in peer_bits(src, kind, n, P, seed)]


def roots(P):
    return sorted({0, 5 % P, P - 1})


def tree_into_guarded(alg, kind, op, ins, w, what, rank=0):
    """One accumulate_f32 reduce_tree call into a guarded, poisoned output (tests/_guard.py), compared on its raw bits."""
    for got in G.launched(w, w.size, DT[kind], lambda out: fmi_amd.reduce_tree(OP[op], alg, out, ins, rank=rank, accumulate_f32=True), what):
        H.assert_bits(got.view(np.uint16), w, kind, op, what)


def check_trees(src, kind, op, n, P, seed, what=""):
    ins = upload(src, kind, n, P, seed)
    tag = f"{what}{src} {kind} {op} P={P} n={n}"
    for r in sorted({0, 1, P - 1}):
        tree_into_guarded(Alg.ALLREDUCE, kind, op, ins, want("allreduce", src, kind, op, n, P, seed)[r], f"allreduce {tag} rank {r}", r)
    for root in roots(P):
        tree_into_guarded(Alg.REDUCE, kind, op, ins, want("reduce", src, kind, op, n, P, seed, root)[0], f"reduce {tag} root {root}", root)
    tree_into_guarded(Alg.REDUCE_LTR, kind, op, ins, want("reduce_ltr", src, kind, op, n, P, seed), f"reduce_ltr {tag}")


def check_scans(src, kind, op, n, P, seed, what="", alias=False):
    """Outputs of their own are guarded and poisoned; aliased ones are the inputs themselves."""
    for alg, family in ((Alg.SCAN, "scan"), (Alg.SCAN_LTR, "scan_ltr")):
        ins = upload(src, kind, n, P, seed)
        w = want(family, src, kind, op, n, P, seed)
        if alias:
            fmi_amd.scan_peers(OP[op], alg, ins, ins, accumulate_f32=True)
            fmi_amd.sync()
            gots = [[read(b) for b in ins]]
        else:
            gots = G.launched_all(w, n, DT[kind], lambda outs: fmi_amd.scan_peers(OP[op], alg, outs, ins, accumulate_f32=True),
                                  f"{what}{family} {src} {kind} {op} P={P} n={n}")
        for got in gots:
            for r in range(P):
                H.assert_bits(got[r].view(np.uint16), w[r], kind, op, f"{what}{family} {src} {kind} {op} P={P} n={n} output {r}")


@pytest.fixture(params=[0, 2], ids=["global_nt", "buffer_sc1"])
def fused_policy(request, device):
    old = fmi_amd.tune_get(Tune.FUSED_POLICY)
    fmi_amd.tune_set(Tune.FUSED_POLICY, request.param)
    yield request.param
    fmi_amd.tune_set(Tune.FUSED_POLICY, old)


@pytest.fixture(params=[1, 0], ids=["one_pass", "block_launches"])
def blocks_one_pass(request, device):
    old = fmi_amd.tune_get(Tune.BLOCKS_ONE_PASS)
    fmi_amd.tune_set(Tune.BLOCKS_ONE_PASS, request.param)
    yield request.param
    fmi_amd.tune_set(Tune.BLOCKS_ONE_PASS, old)


# ---- the fused kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", FUSED_P)
@pytest.mark.parametrize("kind", H.KINDS)
def test_fused_trees(device, kind, P):
    """ALLREDUCE at ranks 0, 1 and P - 1, REDUCE at roots 0, 5 mod P and P - 1, REDUCE_LTR."""
    for n in SIZES:
        check_trees("inputs", kind, "sum", n, P, 31)
        check_trees("cancel", kind, "sum", n, P, 41)
        if P in (5, 16):
            check_trees("inputs", kind, "prod", n, P, 31)


@pytest.mark.parametrize("P", FUSED_P)
@pytest.mark.parametrize("kind", H.KINDS)
def test_fused_scans(device, kind, P):
    """SCAN and SCAN_LTR: every prefix is its own f32 value rounded once."""
    for n in SIZES:
        check_scans("inputs", kind, "sum", n, P, 31)
        check_scans("cancel", kind, "sum", n, P, 41)
        if P in (5, 16):
            check_scans("inputs", kind, "prod", n, P, 31)


@pytest.mark.parametrize("kind", H.KINDS)
def test_outputs_alias_inputs(device, kind):
    n = 2061
    check_scans("cancel", kind, "sum", n, 5, 42, "in place ", alias=True)
    ins = upload("cancel", kind, n, 8, 42)
    fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, ins[2], ins, rank=3, accumulate_f32=True)
    fmi_amd.sync()
    H.assert_bits(read(ins[2]), want("allreduce", "cancel", kind, "sum", n, 8, 42)[3], kind, "sum", "out = ins[2], P = 8")


@pytest.mark.parametrize("kind", H.KINDS)
def test_buffer_and_global_policy(fused_policy, kind):
    """One P per family at both forms of FMI_TUNE_FUSED_POLICY."""
    for n in WIDE_SIZES:
        check_trees("cancel", kind, "sum", n, 5, 43, f"policy {fused_policy} ")
        check_scans("cancel", kind, "sum", n, 8, 43, f"policy {fused_policy} ")


@pytest.mark.parametrize("kind", H.KINDS)
def test_every_bit_pattern(device, kind):
    """Two peers are one combine: acc32 equals the plain definition on all 65,536 patterns against 64 partners each,
    which pins the kernels' widen and narrow code (subnormals, ties, overflow, NaN)."""
    a, b = H.all_patterns()
    ins, out = [bucket(a, kind), bucket(b, kind)], Bucket(a.size, DT[kind])
    for op in ("sum", "prod"):
        fmi_amd.reduce_tree(OP[op], Alg.ALLREDUCE, out, ins, accumulate_f32=True)
        fmi_amd.sync()
        H.assert_bits(read(out), H.combine(op, a, b, kind), kind, op, f"every pattern {kind} {op}")


@pytest.mark.parametrize("kind", H.KINDS)
def test_max_drops_the_flag(device, kind):
    """MAX is a selection: the flag is accepted and the plain kernels run, per-rank bits as before."""
    n, P = 2061, 5
    xs = list(peer_bits("inputs", kind, n, P, 31))
    plain_want = orc.allreduce(xs, H.combiner("max", kind))[0]
    ins, out, plain = upload("inputs", kind, n, P, 31), Bucket(n, DT[kind]), Bucket(n, DT[kind])
    for r in (0, 1, 4):
        fmi_amd.reduce_tree(Op.MAX, Alg.ALLREDUCE, out, ins, rank=r, accumulate_f32=True)
        fmi_amd.reduce_tree(Op.MAX, Alg.ALLREDUCE, plain, ins, rank=r)
        fmi_amd.sync()
        assert np.array_equal(read(out), read(plain)), f"max with the flag, rank {r}"
        H.assert_bits(read(out), plain_want[r], kind, "max", f"max with the flag, rank {r}")


# ---- the fallback: widen, the FMI_F32 program, narrow ------------------------------------------------------------
@pytest.mark.parametrize("P", [17, 33])
@pytest.mark.parametrize("kind", H.KINDS)
def test_fallback_beyond_sixteen_peers(device, kind, P):
    for n in WIDE_SIZES:
        check_trees("cancel", kind, "sum", n, P, 41, "fallback ")
        check_scans("cancel", kind, "sum", n, P, 41, "fallback ")


@pytest.mark.parametrize("kind", H.KINDS)
def test_fallback_unaligned(device, kind):
    """Every bucket a view offset by one element: no 16-B alignment anywhere, the conversions' scalar paths."""
    n, P = 2061, 3
    xs = peer_bits("cancel", kind, n, P, 44)
    view = lambda x: bucket(np.concatenate([np.zeros(1, np.uint16), x]), kind).view(1, n)  # noqa: E731
    ins, out = [view(x) for x in xs], Bucket(n + 1, DT[kind]).view(1, n)
    fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, out, ins, rank=2, accumulate_f32=True)
    fmi_amd.sync()
    H.assert_bits(read(out), want("allreduce", "cancel", kind, "sum", n, P, 44)[2], kind, "sum", "unaligned allreduce")
    fmi_amd.reduce_tree(Op.SUM, Alg.REDUCE_LTR, out, ins, accumulate_f32=True)
    fmi_amd.sync()
    H.assert_bits(read(out), want("reduce_ltr", "cancel", kind, "sum", n, P, 44), kind, "sum", "unaligned reduce_ltr")
    outs = [Bucket(n + 1, DT[kind]).view(1, n) for _ in range(P)]
    fmi_amd.scan_peers(Op.SUM, Alg.SCAN, outs, ins, accumulate_f32=True)
    fmi_amd.sync()
    for r in range(P):
        H.assert_bits(read(outs[r]), want("scan", "cancel", kind, "sum", n, P, 44)[r], kind, "sum", f"unaligned scan {r}")


@pytest.mark.parametrize("kind", H.KINDS)
def test_fallback_blocked_launches_and_one_pass(blocks_one_pass, kind):
    """P = 33 with the inner FMI_F32 program in both modes: the block launches take the scratch arena while the f32
    temporaries are in use."""
    check_trees("cancel", kind, "sum", 2061, 33, 41, f"one_pass={blocks_one_pass} ")
    check_scans("cancel", kind, "sum", 2061, 33, 41, f"one_pass={blocks_one_pass} ")


@pytest.mark.parametrize("kind", H.KINDS)
def test_differential_against_the_f32_kernels(device, kind):
    """The FMI_F32 call on the widened inputs, narrowed on the host, equals the acc32 call."""
    n, P = 2061, 8
    xs = peer_bits("cancel", kind, n, P, 45)
    ins, wide = upload("cancel", kind, n, P, 45), [Bucket.from_numpy(H.widen(x, kind)) for x in xs]
    out, wout = Bucket(n, DT[kind]), Bucket(n, np.float32)
    fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, out, ins, rank=5, accumulate_f32=True)
    fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, wout, wide, rank=5)
    fmi_amd.sync()
    H.assert_bits(read(out), H.narrow(wout.numpy(), kind), kind, "sum", "allreduce against FMI_F32")
    outs, wouts = [Bucket(n, DT[kind]) for _ in range(P)], [Bucket(n, np.float32) for _ in range(P)]
    fmi_amd.scan_peers(Op.SUM, Alg.SCAN, outs, ins, accumulate_f32=True)
    fmi_amd.scan_peers(Op.SUM, Alg.SCAN, wouts, wide)
    fmi_amd.sync()
    for r in range(P):
        H.assert_bits(read(outs[r]), H.narrow(wouts[r].numpy(), kind), kind, "sum", f"scan against FMI_F32, output {r}")


# ---- the communicator: LOCAL transport, every rank compared -----------------------------------------------------
COMM_CASES = [("bf16", "sum", "cancel"), ("f16", "prod", "inputs")]
COMM_N = 4 * 2048 + 5


@pytest.mark.parametrize("N", [4, 8])
@pytest.mark.parametrize("kind,op,src", COMM_CASES)
def test_comm_collectives(device, N, kind, op, src):
    from tests.test_gpu_comm import run_ranks

    n, seed = COMM_N, 46
    xs = peer_bits(src, kind, n, N, seed)
    rts = (0, N - 1)

    def body(c, r):
        new = lambda: Bucket(n, DT[kind])  # noqa: E731
        s, ar, ltr, sc, scl = bucket(xs[r], kind), new(), new(), new(), new()
        c.allreduce(OP[op], s, ar, path=Path.TREE, accumulate_f32=True)
        c.allreduce(OP[op], s, ltr, ordered=True, accumulate_f32=True)
        c.scan(OP[op], s, sc, accumulate_f32=True)
        c.scan(OP[op], s, scl, ordered=True, accumulate_f32=True)
        red, parts = {}, {}
        for root in rts:
            o = new()
            c.reduce(OP[op], s, o if r == root else None, root, accumulate_f32=True)
            fmi_amd.sync()
            red[root] = read(o) if r == root else None
            s2, o2 = bucket(xs[r], kind), new()
            c.reduce(OP[op], s2, o2 if r == root else None, root, sendbuf_partials=True, accumulate_f32=True)
            fmi_amd.sync()
            parts[root] = (read(s2), read(o2) if r == root else None)
        fmi_amd.sync()
        return read(ar), read(ltr), read(sc), read(scl), red, parts

    res = run_ranks(N, body)
    w_ar, w_ltr = want("allreduce", src, kind, op, n, N, seed), want("allreduce_ltr", src, kind, op, n, N, seed)
    w_sc, w_scl = want("scan", src, kind, op, n, N, seed), want("scan_ltr", src, kind, op, n, N, seed)
    for r in range(N):
        tag = f"{kind} {op} N={N} rank {r}"
        H.assert_bits(res[r][0], w_ar[r], kind, op, f"allreduce TREE {tag}")
        H.assert_bits(res[r][1], w_ltr[r], kind, op, f"ordered allreduce {tag}")
        H.assert_bits(res[r][2], w_sc[r], kind, op, f"scan {tag}")
        H.assert_bits(res[r][3], w_scl[r], kind, op, f"ordered scan {tag}")
    for root in rts:
        w_red, w_sends = want("reduce", src, kind, op, n, N, seed, root)
        H.assert_bits(res[root][4][root], w_red, kind, op, f"reduce {kind} {op} N={N} root {root}")
        H.assert_bits(res[root][5][root][1], w_red, kind, op, f"reduce_sendbuf {kind} {op} N={N} root {root}")
        for r in range(N):
            H.assert_bits(res[r][5][root][0], w_sends[r], kind, op, f"{kind} {op} N={N} root {root}: sendbuf of rank {r}")


@pytest.mark.parametrize("kind,op,src", COMM_CASES)
def test_comm_allreduce_direct(device, kind, op, src):
    from tests.test_gpu_comm import run_ranks

    N, n, seed = 4, COMM_N, 47
    xs = peer_bits(src, kind, n, N, seed)

    def body(c, r):
        w, out = c.window(n, DT[kind]), Bucket(n, DT[kind])
        w.upload(xs[r] if kind == "bf16" else xs[r].view(np.float16))
        c.allreduce(OP[op], w, out, path=Path.DIRECT, accumulate_f32=True)
        fmi_amd.sync()
        got = read(out)
        c.window_free(w)
        return got

    res = run_ranks(N, body)
    for r in range(N):
        H.assert_bits(res[r], want("allreduce", src, kind, op, n, N, seed)[r], kind, op, f"allreduce DIRECT rank {r}")


@pytest.mark.parametrize("kind,op,src", COMM_CASES)
def test_comm_allreduce_host(device, kind, op, src):
    """Host arrays through the chunked pipeline, a chunk smaller than n."""
    from tests.test_gpu_comm import run_ranks

    N, n, seed = 2, COMM_N, 48
    xs = peer_bits(src, kind, n, N, seed)

    def body(c, r):
        s = np.array(xs[r]) if kind == "bf16" else np.array(xs[r]).view(np.float16)
        out = np.zeros_like(s)
        c.allreduce_host(OP[op], s, out, chunk=3 * 1024, accumulate_f32=True, dtype=DT[kind])
        return out.view(np.uint16)

    res = run_ranks(N, body)
    for r in range(N):
        H.assert_bits(res[r], want("allreduce", src, kind, op, n, N, seed)[r], kind, op, f"allreduce_host rank {r}")


@pytest.mark.parametrize("kind,op,src", COMM_CASES)
def test_comm_allreduce_twenty_ranks(device, kind, op, src):
    """N = 20: the shard step is the fallback (widen, the 20-peer FMI_F32 allreduce, narrow)."""
    from tests.test_gpu_comm import run_ranks

    N, n, seed = 20, 4099, 49
    xs = peer_bits(src, kind, n, N, seed)

    def body(c, r):
        s, out = bucket(xs[r], kind), Bucket(n, DT[kind])
        c.allreduce(OP[op], s, out, path=Path.TREE, accumulate_f32=True)
        fmi_amd.sync()
        return read(out)

    res = run_ranks(N, body)
    for r in range(N):
        H.assert_bits(res[r], want("allreduce", src, kind, op, n, N, seed)[r], kind, op, f"allreduce N=20 rank {r}")


def test_comm_rccl_path_refuses_the_flag(device):
    """RCCL's reduction has its own order and rounding: FMI_ERR_UNSUPPORTED on every rank, before anything is
    exchanged, and the communicator serves a plain call afterwards."""
    from tests.test_gpu_comm import run_ranks

    N, n, kind, seed = 4, COMM_N, "bf16", 50
    xs = peer_bits("inputs", kind, n, N, seed)

    def body(c, r):
        s, out = bucket(xs[r], kind), Bucket(n, DT[kind])
        with pytest.raises(fmi_amd.FmiError, match="FMI_ERR_UNSUPPORTED.*RCCL"):
            c.allreduce(Op.SUM, s, out, path=Path.RCCL, accumulate_f32=True)
        c.allreduce(Op.SUM, s, out, path=Path.TREE)
        fmi_amd.sync()
        return read(out)

    res = run_ranks(N, body)
    plain = orc.allreduce(list(xs), H.combiner("sum", kind))[0]
    for r in range(N):
        H.assert_bits(res[r], plain[r], kind, "sum", f"plain allreduce after the refusal, rank {r}")


# ---- graph capture ---------------------------------------------------------------------------------------------
def test_graph_capture(device):
    """acc32 calls at P <= 16 on aligned buckets are one fused kernel each: they capture, and replays follow
    re-uploaded inputs. Beyond 16 peers the f32 temporaries refuse the capture."""
    kind, n, P = "bf16", 2061, 8
    st = Stream()
    ins, out = [Bucket(n, DT[kind]) for _ in range(P)], Bucket(n, DT[kind])
    outs = [Bucket(n, DT[kind]) for _ in range(P)]

    def record():
        fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, out, ins, rank=3, stream=st, accumulate_f32=True)
        fmi_amd.scan_peers(Op.SUM, Alg.SCAN, outs, ins, stream=st, accumulate_f32=True)

    g = Graph.capture(st, record)
    try:
        for seed in (51, 52):
            for b, x in zip(ins, peer_bits("cancel", kind, n, P, seed)):
                b.upload(x)
            g.launch(st)
            st.sync()
            H.assert_bits(read(out), want("allreduce", "cancel", kind, "sum", n, P, seed)[3], kind, "sum", f"replay {seed}")
            for r in range(P):
                H.assert_bits(read(outs[r]), want("scan", "cancel", kind, "sum", n, P, seed)[r], kind, "sum",
                              f"replay {seed}: scan output {r}")
    finally:
        g.destroy()
        st.destroy()
    st = Stream()
    wide = [Bucket(n, DT[kind]) for _ in range(17)]
    try:
        with pytest.raises(fmi_amd.FmiError, match="FMI_ERR_UNSUPPORTED.*graph"):
            Graph.capture(st, lambda: fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, out, wide, stream=st, accumulate_f32=True))
    finally:
        st.destroy()


def test_cpp_half_acc_gpu(device):
    """Data<Dev::Bucket<Dev::bfloat16>> through FMI::Communicator with Function(Op, Accumulate::f32)
    (fmi_amd/cpp/tests/test_half_acc.cpp --gpu)."""
    exe = os.path.join(ROOT, "build", "cpp", "test_half_acc")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fmi_amd", "cpp")], check=True)
    out = subprocess.run([exe, "--gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    assert "0 failed checks" in out.stderr
