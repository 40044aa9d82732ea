"""FMI_OP_AVG on the MI355X: the mean over the peers, scaled inside the fused P-way kernels (2..16 peers, aligned
buckets) and by the scale kernel after the unchanged SUM program everywhere else. Every comparison is bit for bit
(a NaN matches any NaN) against tests/_avg.py: oracle.fmi_oracle's event-driven simulation of the SUM, one numpy
multiply by V(1) / V(P), tests/_half.py's narrow for the 16-bit types."""
import functools
import os
import subprocess

import numpy as np
import pytest

import fmi_amd
from fmi_amd import Alg, Bucket, DType, Graph, Op, Stream, Tune
from fmi_amd.comm import Comm, Path, Transport, unique_id
from tests import _avg as G
from tests import _guard
from tests import _half as H
from tests import _half_acc as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"f32": DType.F32, "f64": DType.F64, "f16": DType.F16, "bf16": DType.BF16}
# (kind, accumulate_f32): the six element forms of the fused mean kernels
FORMS = [("f32", False), ("f64", False), ("f16", False), ("bf16", False), ("f16", True), ("bf16", True)]
FORM_IDS = [k + ("_acc32" if a else "") for k, a in FORMS]
FUSED_P = [2, 3, 5, 8, 13, 16]
ERR_INVALID = "FMI_ERR_INVALID"


def bucket(x, kind):
    """A device bucket of these values (16-bit kinds: bit patterns; f16 goes up as np.float16, bf16 as np.uint16)."""
    if not G.is_half(kind):
        return Bucket.from_numpy(np.ascontiguousarray(x))
    b = Bucket(x.size, DT[kind])
    b.upload(x if kind == "bf16" else x.view(np.float16))
    return b


def read(b, kind):
    return b.numpy().view(np.uint16) if G.is_half(kind) else b.numpy()


@functools.lru_cache(maxsize=None)
def peer_values(src, kind, n, P, seed):
    """src "inputs": tests/_avg.py's inputs (edge values included); "cancel": tests/_half_acc.py's cancel_inputs, for
    which the bracketing of S decides the rounded result."""
    xs = A.cancel_inputs(kind, n, P, seed) if src == "cancel" else [G.inputs(kind, n, seed, p) for p in range(P)]
    for x in xs:
        x.setflags(write=False)
    return tuple(xs)


@functools.lru_cache(maxsize=None)
def want(family, src, kind, acc, n, P, seed, root=0):
    """The helper's value(s), computed once per case and left unchanged."""
    return G.expected_avg(family, kind, list(peer_values(src, kind, n, P, seed)), acc, root)


def upload(src, kind, n, P, seed):
    return [bucket(x, kind) for x in peer_values(src, kind, n, P, seed)]


def check_trees(src, kind, acc, n, P, seed, ranks=None, what=""):
    """ALLREDUCE at `ranks` (default: every rank), REDUCE at the same roots, REDUCE_LTR."""
    ins = upload(src, kind, n, P, seed)
    kw = {"accumulate_f32": True} if acc else {}
    tag = f"{what}{src} {kind}{' acc32' if acc else ''} P={P} n={n}"

    def check(alg, w, rank, name):
        """One call into a guarded, poisoned output (tests/_guard.py), compared bit for bit."""
        for got in _guard.launched(w, n, DT[kind], lambda out: fmi_amd.reduce_tree(Op.AVG, alg, out, ins, rank=rank, **kw), name):
            G.assert_same(got.view(np.uint16) if G.is_half(kind) else got, w, kind, name)

    for r in (range(P) if ranks is None else ranks):
        check(Alg.ALLREDUCE, want("allreduce", src, kind, acc, n, P, seed)[r], r, f"allreduce {tag} rank {r}")
        check(Alg.REDUCE, want("reduce", src, kind, acc, n, P, seed, r), r, f"reduce {tag} root {r}")
    check(Alg.REDUCE_LTR, want("reduce_ltr", src, kind, acc, n, P, seed), 0, f"reduce_ltr {tag}")


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
@pytest.mark.parametrize("kind,acc", FORMS, ids=FORM_IDS)
def test_fused(fused_policy, kind, acc, P):
    """Every rank of ALLREDUCE, every root of REDUCE, REDUCE_LTR; tail only, a tile + a group + a ragged tail,
    several tiles; both forms of FMI_TUNE_FUSED_POLICY."""
    for n in G.sizes(kind):
        check_trees("inputs", kind, acc, n, P, 61, what=f"policy {fused_policy} ")
        if acc:
            check_trees("cancel", kind, acc, n, P, 62, what=f"policy {fused_policy} ")


@pytest.mark.parametrize("kind,acc", FORMS, ids=FORM_IDS)
def test_out_aliases_an_input(fused_policy, kind, acc):
    n, P, src = G.sizes(kind)[1], 8, "cancel" if acc else "inputs"
    ins = upload(src, kind, n, P, 63)
    fmi_amd.reduce_tree(Op.AVG, Alg.ALLREDUCE, ins[2], ins, rank=3, **({"accumulate_f32": True} if acc else {}))
    fmi_amd.sync()
    G.assert_same(read(ins[2], kind), want("allreduce", src, kind, acc, n, P, 63)[3], kind, "out = ins[2], P = 8")


def pattern_peers(kind, P):
    """Peer 0: every 16-bit pattern, then 7 tail elements (-0, the smallest and an odd subnormal, the largest finite
    value, the two subnormals negated, +0); the other peers all -0, so that S is every pattern (x + -0 = x)."""
    max_fin = 0x7BFF if kind == "f16" else 0x7F7F
    tail = np.array([0x8000, 0x0001, 0x0003, max_fin, 0x8001, 0x8003, 0x0000], np.uint16)
    x0 = np.concatenate([np.arange(65536, dtype=np.uint32).astype(np.uint16), tail])
    return [x0] + [np.full(x0.size, 0x8000, np.uint16) for _ in range(P - 1)]


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("acc", [False, True], ids=["plain", "acc32"])
@pytest.mark.parametrize("kind", H.KINDS)
def test_every_sixteen_bit_pattern(fused_policy, kind, acc, P):
    """S runs over all 65,536 patterns (-0, subnormals, the ties of halving, +-inf, NaNs), times 1/2 and times
    fl(1/3); the signed-zero trap of a fused multiply-and-narrow sits in the vector body and in the W = 1 tail."""
    xs = pattern_peers(kind, P)
    ins, out = [bucket(x, kind) for x in xs], Bucket(xs[0].size, DT[kind])
    for alg, family in ((Alg.ALLREDUCE, "allreduce"), (Alg.REDUCE_LTR, "reduce_ltr")):
        fmi_amd.reduce_tree(Op.AVG, alg, out, ins, **({"accumulate_f32": True} if acc else {}))
        fmi_amd.sync()
        w = G.expected_avg(family, kind, xs, acc)
        G.assert_same(read(out, kind), w[0] if family == "allreduce" else w, kind, f"every pattern {kind} P={P} {family}")
    assert read(out, kind)[0x8000] == 0x8000 and read(out, kind)[65536] == 0x8000, "-0 x r is -0, body and tail"


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_f32_f64_edge_values(fused_policy, kind):
    """+-0, the smallest and odd subnormals, the largest finite value, +-inf and NaN as S (the other peers hold -0),
    in the vector body and in the tail, at P = 2 (exact halving, ties to even) and P = 3."""
    n = G.sizes(kind)[1]
    for P in (2, 3):
        xs = peer_values("inputs", kind, n, P, 64)
        S = G.sums("allreduce", kind, list(xs))[0]
        e = G.edge_values(kind)
        G.assert_same(S[:e.size], e, kind, "the sum keeps the edge values")
        check_trees("inputs", kind, False, n, P, 64, what="edge values ")
    ins, out = upload("inputs", kind, n, 2, 64), Bucket(n, DT[kind])
    fmi_amd.reduce_tree(Op.AVG, Alg.ALLREDUCE, out, ins)
    fmi_amd.sync()
    got = out.numpy()
    assert np.signbit(got[G.edge_values(kind).size // 2]) and got[G.edge_values(kind).size // 2] == 0, "-0 stays -0"
    assert got[1] == 0 and not np.signbit(got[1]), "half the smallest subnormal ties to even: +0"


def test_overflow_differential(device):
    """f16, four peers holding 60000: the plain sum has overflowed to +inf before the scaling; with f32 accumulation
    the mean is exactly 60000."""
    n = 2061
    x = H.from_float(np.full(n, 60000.0, np.float32), "f16")
    ins, out = [bucket(x, "f16") for _ in range(4)], Bucket(n, DType.F16)
    fmi_amd.reduce_tree(Op.AVG, Alg.ALLREDUCE, out, ins)
    fmi_amd.sync()
    assert (read(out, "f16") == 0x7C00).all()
    fmi_amd.reduce_tree(Op.AVG, Alg.ALLREDUCE, out, ins, accumulate_f32=True)
    fmi_amd.sync()
    assert np.array_equal(read(out, "f16"), x)


def test_one_peer_is_the_copy(device):
    for kind, acc in FORMS:
        x = peer_values("inputs", kind, 1031, 1, 65)[0]
        out = Bucket(x.size, DT[kind])
        fmi_amd.reduce_tree(Op.AVG, Alg.ALLREDUCE, out, [bucket(x, kind)], **({"accumulate_f32": True} if acc else {}))
        fmi_amd.sync()
        assert np.array_equal(read(out, kind).view(np.uint8), np.asarray(x).view(np.uint8)), f"P = 1 {kind}: bits unchanged"


# ---- beyond the fused kernels: the SUM program, then the scale kernel ---------------------------------------------
GENERAL = [("f32", False), ("f64", False), ("bf16", False), ("f16", True), ("bf16", True)]
GENERAL_IDS = [k + ("_acc32" if a else "") for k, a in GENERAL]


def sum_then_scale(kind, alg, ins, rank, n, P):
    out = Bucket(n, DT[kind])
    fmi_amd.reduce_tree(Op.SUM, alg, out, ins, rank=rank)
    fmi_amd.mean_scale(out, P)
    fmi_amd.sync()
    return read(out, kind)


@pytest.mark.parametrize("P", [17, 24, 33, 130])
@pytest.mark.parametrize("kind,acc", GENERAL, ids=GENERAL_IDS)
def test_general_path(blocks_one_pass, kind, acc, P):
    src = "cancel" if acc else "inputs"
    kw = {"accumulate_f32": True} if acc else {}
    algs = [(Alg.ALLREDUCE, "allreduce")] if P == 24 else [(Alg.ALLREDUCE, "allreduce"), (Alg.REDUCE, "reduce"),
                                                           (Alg.REDUCE_LTR, "reduce_ltr")]
    for n in G.sizes(kind)[:2]:
        ins, out = upload(src, kind, n, P, 66), Bucket(n, DT[kind])
        for alg, family in algs:
            for r in (0, P - 1) if family != "reduce_ltr" else (0,):
                fmi_amd.reduce_tree(Op.AVG, alg, out, ins, rank=r, **kw)
                fmi_amd.sync()
                w = want(family, src, kind, acc, n, P, 66, r if family == "reduce" else 0)
                w = w[r] if family == "allreduce" else w
                got = read(out, kind)
                G.assert_same(got, w, kind, f"{family} {kind}{' acc32' if acc else ''} P={P} n={n} rank {r}")
                if not acc:
                    G.assert_same(got, sum_then_scale(kind, alg, ins, r, n, P), kind, f"SUM + mean_scale, {family} P={P}")


@pytest.mark.parametrize("kind,acc", GENERAL, ids=GENERAL_IDS)
def test_unaligned_buckets(device, kind, acc):
    """Every bucket a view offset by one element: the SUM runs as pairwise passes, the scale one element per thread."""
    P, src = 3, "cancel" if acc else "inputs"
    n = G.sizes(kind)[1]
    xs = peer_values(src, kind, n, P, 67)
    pad = np.zeros(1, xs[0].dtype)
    ins = [bucket(np.concatenate([pad, x]), kind).view(1, n) for x in xs]
    out = Bucket(n + 1, DT[kind]).view(1, n)
    kw = {"accumulate_f32": True} if acc else {}
    for alg, family, r in ((Alg.ALLREDUCE, "allreduce", 2), (Alg.REDUCE, "reduce", 1), (Alg.REDUCE_LTR, "reduce_ltr", 0)):
        fmi_amd.reduce_tree(Op.AVG, alg, out, ins, rank=r, **kw)
        fmi_amd.sync()
        w = want(family, src, kind, acc, n, P, 67, r if family == "reduce" else 0)
        G.assert_same(read(out, kind), w[r] if family == "allreduce" else w, kind, f"unaligned {family} {kind}")


# ---- fmi_dev_mean_scale alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("kind", G.KINDS)
def test_mean_scale(device, kind, offset):
    if G.is_half(kind):
        x = pattern_peers(kind, 1)[0]
        val = H.widen(x, kind)
    else:
        n = G.sizes(kind)[1]
        x = np.array(peer_values("inputs", kind, n, 1, 68)[0])
        x[n - 5:] = G.edge_values(kind)[1:6]
        val = x
    for P in (2, 3, 7, 1):
        whole = bucket(np.concatenate([np.zeros(offset, x.dtype), x]), kind)
        b = whole.view(offset, x.size)
        fmi_amd.mean_scale(b, P)
        fmi_amd.sync()
        G.assert_same(read(b, kind), G.scale(val, kind, P), kind, f"mean_scale {kind} P={P} offset {offset}")
        if offset:
            assert read(whole, kind)[0] == 0, "the element before the view is untouched"
    fmi_amd.mean_scale(Bucket(8, DT[kind]), 3, n=0)


def test_mean_scale_refuses_integers(device):
    b = Bucket.from_numpy(np.arange(8, dtype=np.int32))
    with pytest.raises(fmi_amd.FmiError, match=f"{ERR_INVALID}.*integer"):
        fmi_amd.mean_scale(b, 2)
    assert np.array_equal(b.numpy(), np.arange(8, dtype=np.int32))


# ---- refusals ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_buffers_alone(device):
    from tests.test_gpu_comm import run_ranks

    n = 1031
    x, y = peer_values("inputs", "f32", n, 2, 69)
    a, b, out = bucket(x, "f32"), bucket(y, "f32"), Bucket.from_numpy(np.zeros(n, np.float32))
    calls = [lambda: fmi_amd.reduce_pair(Op.AVG, a, b), lambda: fmi_amd.combine(Op.AVG, out, a, b),
             lambda: fmi_amd.reduce_pair_batch(Op.AVG, [(a, b)]),
             lambda: fmi_amd.scan_peers(Op.AVG, Alg.SCAN, [out, Bucket(n, np.float32)], [a, b]),
             lambda: fmi_amd.reduce_tree(Op.AVG, Alg.ALLREDUCE, Bucket(8, np.int32), [Bucket(8, np.int32)] * 2)]
    for call in calls:
        with pytest.raises(fmi_amd.FmiError, match=f"{ERR_INVALID}.*FMI_OP_AVG"):
            call()
    fmi_amd.sync()
    G.assert_same(a.numpy(), x, "f32", "a untouched")
    G.assert_same(b.numpy(), y, "f32", "b untouched")
    assert not out.numpy().any()

    def body(c, r):
        s, o = bucket(peer_values("inputs", "f32", n, 2, 69)[r], "f32"), Bucket.from_numpy(np.zeros(n, np.float32))
        with pytest.raises(fmi_amd.FmiError, match=f"{ERR_INVALID}.*FMI_OP_AVG.*fmi_comm_scan|{ERR_INVALID}.*fmi_comm_scan.*FMI_OP_AVG"):
            c.scan(Op.AVG, s, o)
        for ordered in (False, True):
            with pytest.raises(fmi_amd.FmiError, match=f"{ERR_INVALID}.*fmi_comm_reduce_sendbuf.*FMI_OP_AVG"):
                c.reduce(Op.AVG, s, o if r == 0 else None, 0, ordered=ordered, sendbuf_partials=True)
        with pytest.raises(fmi_amd.FmiError, match=f"{ERR_INVALID}.*FMI_OP_AVG.*integer"):
            c.allreduce(Op.AVG, Bucket(8, np.int32), Bucket(8, np.int32))
        fmi_amd.sync()
        return s.numpy(), o.numpy()

    for r, (s, o) in enumerate(run_ranks(2, body)):
        G.assert_same(s, peer_values("inputs", "f32", n, 2, 69)[r], "f32", "send untouched")
        assert not o.any()


# ---- the communicator: LOCAL transport, every rank compared -----------------------------------------------------
COMM_N = 4 * 2048 + 5
COMM_FORMS = [("bf16", True, "cancel"), ("f32", False, "inputs")]
COMM_IDS = ["bf16_acc32", "f32"]


def host_array(x, kind):
    return np.array(x) if kind != "f16" else np.array(x).view(np.float16)


@pytest.mark.parametrize("N", [4, 8, 20])
@pytest.mark.parametrize("kind,acc,src", COMM_FORMS, ids=COMM_IDS)
def test_comm_collectives(device, N, kind, acc, src):
    from tests.test_gpu_comm import run_ranks

    n, seed = COMM_N, 70
    xs = peer_values(src, kind, n, N, seed)
    rts = (1, N - 1)
    kw = {"accumulate_f32": True} if acc else {}

    def body(c, r):
        new = lambda: Bucket(n, DT[kind])  # noqa: E731
        s, tree, ltr = bucket(xs[r], kind), new(), new()
        c.allreduce(Op.AVG, s, tree, path=Path.TREE, **kw)
        c.allreduce(Op.AVG, s, ltr, ordered=True, **kw)
        w, direct = c.window(n, DT[kind]), new()
        w.upload(host_array(xs[r], kind))
        c.allreduce(Op.AVG, w, direct, path=Path.DIRECT, **kw)
        red = {}
        for root in rts:
            o = new()
            c.reduce(Op.AVG, s, o if r == root else None, root, **kw)
            fmi_amd.sync()
            red[root] = read(o, kind) if r == root else None
        fmi_amd.sync()
        got = read(tree, kind), read(ltr, kind), read(direct, kind), red, read(s, kind)
        c.window_free(w)
        h = host_array(xs[r], kind)
        hout = np.zeros_like(h)
        c.allreduce_host(Op.AVG, h, hout, chunk=3 * 1024, dtype=DT[kind], **kw)
        return got + (hout.view(np.uint16) if G.is_half(kind) else hout,)

    res = run_ranks(N, body)
    w_ar, w_ltr = want("allreduce", src, kind, acc, n, N, seed), want("allreduce_ltr", src, kind, acc, n, N, seed)
    for r in range(N):
        tag = f"{kind}{' acc32' if acc else ''} N={N} rank {r}"
        G.assert_same(res[r][0], w_ar[r], kind, f"allreduce TREE {tag}")
        G.assert_same(res[r][1], w_ltr[r], kind, f"ordered allreduce {tag}")
        G.assert_same(res[r][2], w_ar[r], kind, f"allreduce DIRECT {tag}")
        G.assert_same(res[r][4], xs[r], kind, f"send untouched {tag}")
        G.assert_same(res[r][5], w_ar[r], kind, f"allreduce_host {tag}")
    for root in rts:
        G.assert_same(res[root][3][root], want("reduce", src, kind, acc, n, N, seed, root), kind,
                      f"reduce {kind} N={N} root {root}")


@pytest.mark.parametrize("path", [Path.TREE, Path.RCCL], ids=["tree", "rccl"])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_comm_one_rank_exchange(device, kind, path):
    """A one-rank RCCL communicator running the full exchange: the mean of one bucket is its own bits (path RCCL:
    the reduce-scatter against itself with SUM, a scale by 1, the all-gather)."""
    n = 4099
    x = peer_values("inputs", kind, n, 1, 71)[0]
    c = Comm(unique_id(Transport.RCCL), 1, 0, timeout_s=120)
    fmi_amd.tune_set(Tune.COMM_ONE_RANK_EXCHANGE, 1)
    try:
        s, out = bucket(x, kind), Bucket(n, DT[kind])
        c.allreduce(Op.AVG, s, out, path=path)
        c.sync()
        assert np.array_equal(read(out, kind).view(np.uint8), np.asarray(x).view(np.uint8)), f"one rank, {kind}"
    finally:
        fmi_amd.tune_set(Tune.COMM_ONE_RANK_EXCHANGE, 0)
        c.destroy()


# ---- graph capture ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,acc,P,alg,family", [("bf16", True, 8, Alg.ALLREDUCE, "allreduce"),
                                                   ("f32", False, 8, Alg.ALLREDUCE, "allreduce"),
                                                   ("f32", False, 33, Alg.REDUCE, "reduce")],
                         ids=["bf16_acc32_p8", "f32_p8", "f32_p33_reduce"])
def test_graph_capture(device, kind, acc, P, alg, family):
    """One fused kernel at P <= 16; beyond, the SUM program's capturable form and the in-place scale: replays follow
    re-uploaded inputs."""
    n, src, rank = G.sizes(kind)[1], "cancel" if acc else "inputs", 3
    st = Stream()
    ins, out = [Bucket(n, DT[kind]) for _ in range(P)], Bucket(n, DT[kind])
    kw = {"accumulate_f32": True} if acc else {}
    g = Graph.capture(st, lambda: fmi_amd.reduce_tree(Op.AVG, alg, out, ins, rank=rank, stream=st, **kw))
    try:
        for seed in (72, 73):
            for b, x in zip(ins, peer_values(src, kind, n, P, seed)):
                b.upload(host_array(x, kind))
            g.launch(st)
            st.sync()
            w = want(family, src, kind, acc, n, P, seed, rank if family == "reduce" else 0)
            G.assert_same(read(out, kind), w[rank] if family == "allreduce" else w, kind, f"replay {seed}")
    finally:
        g.destroy()
        st.destroy()


def test_graph_capture_refused_beyond_sixteen_peers_with_acc32(device):
    """bf16 with f32 accumulation at 17 peers needs the f32 temporaries: the capture fails, and the stream is replaced."""
    n = 2061
    out, wide = Bucket(n, DType.BF16), [Bucket(n, DType.BF16) for _ in range(17)]
    st = Stream()
    try:
        with pytest.raises(fmi_amd.FmiError, match="FMI_ERR_UNSUPPORTED.*graph"):
            Graph.capture(st, lambda: fmi_amd.reduce_tree(Op.AVG, Alg.ALLREDUCE, out, wide, stream=st, accumulate_f32=True))
    finally:
        st.destroy()
    st = Stream()
    try:
        xs = peer_values("cancel", "bf16", n, 17, 74)
        for b, x in zip(wide, xs):
            b.upload(x)
        fmi_amd.reduce_tree(Op.AVG, Alg.ALLREDUCE, out, wide, stream=st, accumulate_f32=True)
        st.sync()
        G.assert_same(read(out, "bf16"), want("allreduce", "cancel", "bf16", True, n, 17, 74)[0], "bf16", "a fresh stream serves")
    finally:
        st.destroy()


# ---- C++ ------------------------------------------------------------------------------------------------------
def test_cpp_avg_gpu(device):
    """Data<Dev::Bucket<float>> and Data<Dev::Bucket<Dev::bfloat16>> through FMI::Communicator with Op::avg
    (fmi_amd/cpp/tests/test_avg.cpp --gpu): the sum finished by fmi_dev_mean_scale."""
    exe = os.path.join(ROOT, "build", "cpp", "test_avg")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fmi_amd", "cpp")], check=True)
    out = subprocess.run([exe, "--gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    assert "0 failed checks" in out.stderr
