"""The scaled FP8 reduction on the GPU (fmi_dev_reduce_tree_scaled, fmi_comm_allreduce_scaled), bit for bit against
tests/_fp8_scaled.py: bytes with F.assert_bits, f32 output and amax on their uint32 views, a NaN matching any NaN."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fmi_amd
from fmi_amd import Alg, Bucket, DType, Graph, Stream, Tune
from tests import _fp8 as F
from tests import _fp8_scaled as FS
from tests import _guard as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"e4m3": DType.F8E4M3, "e5m2": DType.F8E5M2}
# three 256-thread tiles of 16-B lane groups plus a ragged tail: more than one workgroup in the amax reduction
N_FUSED = 3 * 4096 + 7
SIZES = (N_FUSED, 1, 15, 16)
FUSED_P = [2, 3, 5, 8, 13, 16]
SEED = 7
# (name, oracle family, Alg, root as a function of P)
ALGS = {
    "allreduce": ("allreduce", Alg.ALLREDUCE, lambda P: 0),
    "reduce_root0": ("reduce", Alg.REDUCE, lambda P: 0),
    "reduce_rootlast": ("reduce", Alg.REDUCE, lambda P: P - 1),
    "reduce_ltr": ("reduce_ltr", Alg.REDUCE_LTR, lambda P: 0),
}
MAX_BYTE = {"e4m3": 0x7E, "e5m2": 0x7B}  # the largest finite value, positive


@functools.lru_cache(maxsize=None)
def inputs(kind, P, n=N_FUSED, seed=SEED):
    return tuple(F.synthetic(kind, n, seed, p) for p in range(P))


def bucket(bits, kind, offset=0):
    bits = np.asarray(bits, np.uint8)
    b = Bucket(bits.size + offset, DT[kind])
    b.upload(np.concatenate([np.zeros(offset, np.uint8), bits]))
    return b.view(offset, bits.size) if offset else b


def out_bucket(n, kind, out, offset=0):
    """A bucket for the result, holding other values beforehand."""
    b = Bucket(n + offset, DT[kind] if out == "same" else DType.F32)
    b.upload(np.full(n + offset, 0x55, np.uint8) if out == "same" else np.full(n + offset, 1.5, np.float32))
    return b.view(offset, n) if offset else b


def f32_bucket(values):
    return Bucket.from_numpy(np.atleast_1d(np.asarray(values, np.float32)))


def word(bits=0):
    return Bucket.from_numpy(np.array([bits], np.uint32).view(np.float32))


def read_out(b, out):
    return b.numpy() if out == "same" else b.numpy().view(np.float32)


def read_word(b):
    return int(b.numpy().view(np.uint32)[0])


def run(alg, kind, xs, s, t, out, root=0, amax_bits=0, offset=0, stream=None, want=None, what=""):
    """One call on fresh buckets: (output, amax bits or None). amax_bits None: amax = NULL. The output and the one-float
    amax slot sit inside guarded allocations (tests/_guard.py): no byte around them may change. With `want` the output is
    poisoned under the poison rule, the call made once per poison, and no element may be left unwritten."""
    n = xs[0].size
    ins = [bucket(x, kind, offset) for x in xs]
    dtype, off = (DT[kind], offset) if out == "same" else (DType.F32, 0)
    for o in (G.guarded_runs(want, n, dtype, off) if want is not None else [G.Guarded(n, dtype, off)]):
        am = None if amax_bits is None else G.Guarded(1, DType.F32, 7).load([np.array([amax_bits], np.uint32)])
        fmi_amd.reduce_tree_scaled(alg, o.b, ins, f32_bucket(s), None if t is None else f32_bucket(t), None if am is None else am.b,
                                   rank=root, stream=stream)
        fmi_amd.sync()
        got = o.read(want, what)
        got_amax = None if am is None else int(am.read(None, f"{what} amax").view(np.uint32)[0])
        if want is not None:
            FS.assert_out(got, want, kind, out, what)
    return got, got_amax


def check(name, kind, xs, s, t, out, amax_bits=0, offset=0, what=""):
    family, alg, root_of = ALGS[name]
    root = root_of(len(xs))
    want, want_amax, _ = FS.expected_scaled(family, kind, xs, s, t, out, root)
    tag = f"{what} {kind} {name} P={len(xs)} n={xs[0].size} out={out} t={t}"
    got, got_amax = run(alg, kind, xs, s, t, out, root, amax_bits, offset, want=want, what=tag)
    FS.assert_out(got, want, kind, out, tag)
    if amax_bits is not None:
        FS.assert_amax(got_amax, FS.fold_amax(amax_bits, want_amax), tag)


# ---- the fused kernels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["same", "f32"])
@pytest.mark.parametrize("P", FUSED_P)
@pytest.mark.parametrize("name", list(ALGS))
@pytest.mark.parametrize("kind", F.KINDS)
def test_fused(device, kind, name, P, out):
    """The f32 output pins the order and any contraction (tests/test_fp8_scaled_cpu.py); the 8-bit one the narrowing."""
    s = FS.scales(P)
    for n in SIZES:
        xs = [x[:n] for x in inputs(kind, P)]
        check(name, kind, xs, s, FS.T_OUT, out)
        check(name, kind, xs, s, None, out, amax_bits=None)  # out_scale = NULL, amax = NULL


@pytest.mark.parametrize("policy", [0, 2])
def test_fused_both_access_policies(device, policy):
    """The global (0) and the buffer (2) accesses at peer counts the default would send the other way."""
    fmi_amd.tune_set(Tune.FUSED_POLICY, policy)
    try:
        for kind in F.KINDS:
            for P in (3, 8):
                for out in ("same", "f32"):
                    check("allreduce", kind, list(inputs(kind, P)), FS.scales(P), FS.T_OUT, out, what=f"policy {policy}")
    finally:
        fmi_amd.tune_set(Tune.FUSED_POLICY, 1)


@pytest.mark.parametrize("where", [0, 4096 + 1000, N_FUSED - 1])
@pytest.mark.parametrize("kind", F.KINDS)
def test_amax_sees_every_part_of_the_bucket(device, kind, where):
    """The maximum |S| sits in element 0, in the middle tile, in the LAST tail element: every peer holds the largest
    finite value there and every scale is positive."""
    P = 5
    xs = [x.copy() for x in inputs(kind, P)]
    for x in xs:
        x[where] = MAX_BYTE[kind]
    s = FS.scales(P)
    _, want_amax, S = FS.expected_scaled("allreduce", kind, xs, s, None, "f32")
    assert int(np.argmax(np.abs(S))) == where and np.sum(np.abs(S) == np.abs(S[where])) == 1
    for out in ("same", "f32"):
        check("allreduce", kind, xs, s, FS.T_OUT, out, what=f"amax at {where}")
        check("reduce_ltr", kind, xs, s, None, out, what=f"amax at {where}")


@pytest.mark.parametrize("kind", F.KINDS)
def test_amax_presets_and_accumulation(device, kind):
    P = 8
    xs, s = list(inputs(kind, P)), FS.scales(P)
    above = int(np.array([1e30], np.float32).view(np.uint32)[0])
    check("allreduce", kind, xs, s, FS.T_OUT, "same", amax_bits=0, what="preset 0")
    got, amax = run(Alg.ALLREDUCE, kind, xs, s, FS.T_OUT, "same", amax_bits=above)
    assert amax == above, "a preset above the maximum stays"
    # accumulated over two buckets: the second one's values are twice as large
    ys = [F.synthetic(kind, N_FUSED, SEED + 1, p) for p in range(P)]
    am = word(0)
    ins_x, ins_y = [bucket(x, kind) for x in xs], [bucket(y, kind) for y in ys]
    o = out_bucket(N_FUSED, kind, "f32")
    fmi_amd.reduce_tree_scaled(Alg.ALLREDUCE, o, ins_x, f32_bucket(s), None, am)
    fmi_amd.sync()
    a1 = FS.expected_scaled("allreduce", kind, xs, s, None, "f32")[1]
    FS.assert_amax(read_word(am), a1, "first bucket")
    fmi_amd.reduce_tree_scaled(Alg.ALLREDUCE, o, ins_y, f32_bucket(2 * s), None, am)
    fmi_amd.sync()
    a2 = FS.expected_scaled("allreduce", kind, ys, 2 * s, None, "f32")[1]
    assert a2 != a1
    FS.assert_amax(read_word(am), max(a1, a2), "two buckets")


@pytest.mark.parametrize("kind", F.KINDS)
def test_nan_sum_gives_nan_amax(device, kind):
    P = 5
    xs = [x.copy() for x in inputs(kind, P)]
    if kind == "e5m2":
        xs[1][4096 + 33], xs[3][4096 + 33] = 0x7C, 0xFC  # +inf and -inf
    else:
        xs[2][4096 + 33] = 0x7F  # the NaN byte
    s = FS.scales(P)
    want_amax = FS.expected_scaled("allreduce", kind, xs, s, None, "f32")[1]
    assert (want_amax & 0x7FFFFFFF) > 0x7F800000
    for out in ("same", "f32"):
        check("allreduce", kind, xs, s, FS.T_OUT, out, what="NaN in S")


@pytest.mark.parametrize("kind", F.KINDS)
def test_narrowing_does_not_saturate(device, kind):
    """Partial sums beyond the largest finite value that come back in range, then an output scale that takes S * t
    beyond it: inf (e5m2) or NaN (e4m3) bytes, never the largest finite value."""
    P = 8
    xs, s = F.overflow_inputs(kind, N_FUSED, P, SEED), np.ones(P, np.float32)
    t = np.float32(2.0 ** 20)
    want = FS.expected_scaled("allreduce", kind, xs, s, t, "same")[0]
    w = F.widen(want, kind)
    assert np.mean(~np.isfinite(w)) > 0.5 and not np.any(np.abs(w) == F.MAX_FINITE[kind])
    for name in ("allreduce", "reduce_rootlast", "reduce_ltr"):
        check(name, kind, xs, s, t, "same", what="overflow")
        check(name, kind, xs, s, None, "same", what="partials overflow")


# ---- beyond the fused kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["same", "f32"])
@pytest.mark.parametrize("P", [1, 16, 17, 33])
@pytest.mark.parametrize("kind", F.KINDS)
def test_fallback_peer_counts(device, kind, P, out):
    """P = 1 (not a copy), and 16 (fused) beside 17 and 33 (f32 temporaries): each equal to the oracle."""
    xs, s = list(inputs(kind, P)), FS.scales(P)
    for name in ALGS:
        check(name, kind, xs, s, FS.T_OUT, out, what="fallback")
    check("allreduce", kind, [x[:15] for x in xs], s, None, out, amax_bits=None, what="fallback")


@pytest.mark.parametrize("out", ["same", "f32"])
@pytest.mark.parametrize("kind", F.KINDS)
def test_fallback_unaligned(device, kind, out):
    xs, s = list(inputs(kind, 5)), FS.scales(5)
    for name in ALGS:
        check(name, kind, xs, s, FS.T_OUT, out, offset=1, what="1-byte offset")


# ---- graph capture -------------------------------------------------------------------------------------------------
def test_graph_replay_reads_new_scales(device):
    kind, P, n = "e4m3", 8, N_FUSED
    xs = list(inputs(kind, P))
    ins, o = [bucket(x, kind) for x in xs], out_bucket(n, kind, "f32")
    s_old, s_new = FS.scales(P), FS.scales(2 * P)[P:]
    assert not np.array_equal(s_old, s_new)
    sc, t, am = f32_bucket(s_old), f32_bucket(FS.T_OUT), word(0)
    fmi_amd.sync()
    st = Stream()
    g = Graph.capture(st, lambda: fmi_amd.reduce_tree_scaled(Alg.ALLREDUCE, o, ins, sc, t, am, stream=st))
    try:
        for s in (s_old, s_new):
            sc.upload(s)
            am.upload(np.zeros(1, np.float32))
            g.launch(st)
            st.sync()
            want, want_amax, _ = FS.expected_scaled("allreduce", kind, xs, s, FS.T_OUT, "f32")
            FS.assert_f32_bits(read_out(o, "f32"), want, "graph replay")
            FS.assert_amax(read_word(am), want_amax, "graph replay")
    finally:
        g.destroy()
        st.destroy()


# ---- the communicator: LOCAL transport, every rank compared ----------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("N", [2, 3, 8])
@pytest.mark.parametrize("kind", F.KINDS)
def test_comm_allreduce_scaled(device, kind, N, ragged):
    from tests.test_gpu_comm import run_ranks

    n = 64 * N * 3 + (5 if ragged else 0)
    xs, s = [F.synthetic(kind, n, 81, r) for r in range(N)], FS.scales(N)

    def body(c, r):
        send, res = bucket(xs[r], kind), {}
        for out in ("same", "f32"):
            for ordered in (False, True):
                recv, am = out_bucket(n, kind, out), word(0)
                c.allreduce_scaled(send, f32_bucket(s[r]), recv, f32_bucket(FS.T_OUT), am, ordered=ordered)
                fmi_amd.sync()
                res[out, ordered] = (read_out(recv, out), read_word(am))
        recv = out_bucket(n, kind, "f32")
        c.allreduce_scaled(send, f32_bucket(s[r]), recv)  # out_scale = NULL, amax = NULL
        fmi_amd.sync()
        res["plain"] = read_out(recv, "f32")
        res["send"] = send.numpy()
        return res

    res = run_ranks(N, body)
    for out in ("same", "f32"):
        for ordered in (False, True):
            want, want_amax, _ = FS.expected_scaled("allreduce_ltr" if ordered else "allreduce", kind, xs, s, FS.T_OUT, out)
            for r in range(N):
                tag = f"{kind} N={N} n={n} out={out} ordered={ordered} rank {r}"
                FS.assert_out(res[r][out, ordered][0], want, kind, out, tag)
                FS.assert_amax(res[r][out, ordered][1], want_amax, tag)
    want = FS.expected_scaled("allreduce", kind, xs, s, None, "f32")[0]
    for r in range(N):
        FS.assert_f32_bits(res[r]["plain"], want, f"{kind} N={N} no out_scale, no amax, rank {r}")
        assert np.array_equal(res[r]["send"], xs[r]), f"send of rank {r} was modified"


@pytest.mark.parametrize("kind", F.KINDS)
def test_comm_padding_does_not_reach_amax(device, kind):
    """Rank 0's scale is inf and no element is zero: every sum is +-inf, amax is inf. A zero of the shard grid's
    padding times inf would be a NaN, and a NaN wins the maximum."""
    from tests.test_gpu_comm import run_ranks

    N = 3
    n = 64 * N * 3 + 5
    xs = [F.synthetic(kind, n, 83, r) for r in range(N)]
    xs = [np.where((x & 0x7F) == 0, np.uint8(0x30), x) for x in xs]
    s = FS.scales(N)
    s[0] = np.inf

    def body(c, r):
        recv, am = out_bucket(n, kind, "f32"), word(0)
        c.allreduce_scaled(bucket(xs[r], kind), f32_bucket(s[r]), recv, None, am)
        fmi_amd.sync()
        return read_out(recv, "f32"), read_word(am)

    res = run_ranks(N, body)
    want, want_amax, _ = FS.expected_scaled("allreduce", kind, xs, s, None, "f32")
    assert want_amax == 0x7F800000
    for r in range(N):
        FS.assert_f32_bits(res[r][0], want, f"rank {r}")
        assert res[r][1] == 0x7F800000, f"rank {r}: amax 0x{res[r][1]:08x}"


def test_one_rank_communicator_runs_the_p1_form(device):
    from tests.test_gpu_comm import run_ranks

    kind, n = "e5m2", 1000
    x, s = F.synthetic(kind, n, 85, 0), FS.scales(2)[1:]

    def body(c, r):
        recv, am = out_bucket(n, kind, "same"), word(0)
        c.allreduce_scaled(bucket(x, kind), f32_bucket(s), recv, f32_bucket(FS.T_OUT), am)
        fmi_amd.sync()
        return recv.numpy(), read_word(am)

    got, amax = run_ranks(1, body)[0]
    want, want_amax, _ = FS.expected_scaled("allreduce", kind, [x], s, FS.T_OUT, "same")
    F.assert_bits(got, want, kind, "one rank")
    FS.assert_amax(amax, want_amax, "one rank")


# ---- the Python layer's own checks -------------------------------------------------------------------------------
def test_python_layers_refuse_wrong_buckets(device):
    xs = [bucket(x[:64], "e4m3") for x in inputs("e4m3", 2)]
    with pytest.raises(ValueError):
        fmi_amd.reduce_tree_scaled(Alg.ALLREDUCE, Bucket(64, DType.BF16), xs, f32_bucket(FS.scales(2)))
    with pytest.raises(ValueError):
        fmi_amd.reduce_tree_scaled(Alg.ALLREDUCE, Bucket(64, DType.F32), xs, f32_bucket(FS.scales(1)))
    with pytest.raises(fmi_amd.FmiError, match="scan algorithm"):
        fmi_amd.reduce_tree_scaled(Alg.SCAN, Bucket(64, DType.F32), xs, f32_bucket(FS.scales(2)))


def test_torch_glue(device):
    """HipEngine.reduce_tree_scaled on torch float8 device tensors and float32 scale tensors (a child process: torch must
    be loaded before the library) equals the definition."""
    r = subprocess.run([sys.executable, "-u", "-m", "tests._fp8_scaled_torch_worker"], cwd=ROOT, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0 and "fp8 scaled torch glue ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
