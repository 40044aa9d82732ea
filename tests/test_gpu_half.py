"""FMI_F16 / FMI_BF16 buckets on the MI355X: the pairwise family, the fused P-way kernels, the forms left to the
stepwise path, the communicator, the synthetic fill, the torch glue and the C++ surface. Every comparison is on the
16 raw bits against tests/_half.py's definition (widen to f32, op, round to nearest even; max / min keep one
operand's bits), with the one relaxation that a NaN made by sum / prod matches any NaN. Expected values of P-way
programs come from the oracle's event-driven simulation with that combine as `f`."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fmi_amd
from fmi_amd import Alg, Bucket, DType, Op, Tune
from fmi_amd.comm import Comm, Path, Transport, unique_id
from oracle import fmi_oracle as orc
from tests import _half as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"f16": DType.F16, "bf16": DType.BF16}
OP = {"sum": Op.SUM, "prod": Op.PROD, "max": Op.MAX, "min": Op.MIN}
TILE = 4 * 256 * 8  # one whole pairwise tile: unroll 4 x 256 threads x 8 elements
PAIR_SIZES = [0, 1, 7, 8, 9, 15, 16, 17, TILE - 1, TILE, TILE + 8 + 3, 2 * TILE + 13]
FUSED_SIZES = [1, 7, 8, 2061, 3 * 2048 + 11]  # 2061: one 256-thread tile + one vector + a tail


def bucket(bits, kind):
    """A device bucket holding these bit patterns (f16 goes up as np.float16, bf16 as its raw np.uint16)."""
    b = Bucket(bits.size, DT[kind])
    b.upload(bits if kind == "bf16" else bits.view(np.float16))
    return b


def read(b):
    return b.numpy().view(np.uint16)


def test_bucket_dtypes(device):
    assert Bucket(8, np.float16).dtype is DType.F16 and Bucket(8, DType.BF16).itemsize == 2
    assert Bucket.from_numpy(np.zeros(8, np.float16)).dtype is DType.F16
    assert Bucket.from_numpy(np.zeros(8, np.uint16)).dtype is DType.U16
    assert Bucket(8, DType.BF16).numpy().dtype == np.uint16


@pytest.mark.parametrize("op", H.OPS)
@pytest.mark.parametrize("kind", H.KINDS)
def test_pairwise_sizes_and_edges(device, kind, op):
    for n in PAIR_SIZES:
        a, b = H.inputs(kind, n, seed=42, peer=0), H.inputs(kind, n, seed=42, peer=1)
        da, db = bucket(a, kind), bucket(b, kind)
        fmi_amd.reduce_pair(OP[op], da, db)
        fmi_amd.sync()
        H.assert_bits(read(da), H.combine(op, a, b, kind), kind, op, f"{kind} {op} n={n}")
        H.assert_bits(read(db), b, kind, "max", f"`in` untouched, n={n}")
        out = Bucket(n, DT[kind])
        fmi_amd.combine(OP[op], out, db, bucket(a, kind))  # the other operand order
        fmi_amd.sync()
        H.assert_bits(read(out), H.combine(op, b, a, kind), kind, op, f"{kind} {op} combine n={n}")


@pytest.fixture(scope="module")
def patterns():
    a, b = H.all_patterns(1 << 22)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@pytest.mark.parametrize("kind", H.KINDS)
def test_pairwise_all_bit_patterns(device, patterns, kind):
    """All 65,536 patterns against 64 permutations of them (2^22 elements) through reduce_pair: pins the packed
    convert's rounding, NaN and subnormal behaviour on the hardware (a flushed subnormal would show here)."""
    a, b = patterns
    db = bucket(b, kind)
    for op in H.OPS:
        da = bucket(a, kind)
        fmi_amd.reduce_pair(OP[op], da, db)
        fmi_amd.sync()
        H.assert_bits(read(da), H.combine(op, a, b, kind), kind, op, f"{kind} {op} all patterns")
        da.free()


@pytest.mark.parametrize("kind", H.KINDS)
def test_pairwise_unaligned_views_and_alias(device, kind):
    n = 4099
    for off in (1, 3, 5):
        for op in H.OPS:
            a, b = H.inputs(kind, n + 8, seed=5, peer=0), H.inputs(kind, n + 8, seed=5, peer=1)
            da, db = bucket(a, kind), bucket(b, kind)
            fmi_amd.reduce_pair(OP[op], da.view(off, n), db.view(off, n))  # the scalar kernel
            fmi_amd.sync()
            want = a.copy()
            want[off:off + n] = H.combine(op, a[off:off + n], b[off:off + n], kind)
            H.assert_bits(read(da), want, kind, op, f"{kind} {op} offset {off}: outside the view untouched")
    for op in H.OPS:
        a = H.inputs(kind, TILE + 11, seed=6, peer=0)
        da = bucket(a, kind)
        fmi_amd.reduce_pair(OP[op], da, da)  # in place, aliased
        fmi_amd.sync()
        H.assert_bits(read(da), H.combine(op, a, a, kind), kind, op, f"{kind} {op} reduce_pair(a, a)")


@pytest.mark.parametrize("kind", H.KINDS)
def test_reduce_pair_batch(device, kind):
    sizes = [1, 8, 2061, 8192, 8205]
    for op in H.OPS:
        xs = [(H.inputs(kind, n, seed=8, peer=2 * k), H.inputs(kind, n, seed=8, peer=2 * k + 1)) for k, n in enumerate(sizes)]
        pairs = [(bucket(a, kind), bucket(b, kind)) for a, b in xs]
        fmi_amd.reduce_pair_batch(OP[op], pairs)
        fmi_amd.sync()
        for (a, b), (da, db) in zip(xs, pairs):
            H.assert_bits(read(da), H.combine(op, a, b, kind), kind, op, f"{kind} {op} batch n={a.size}")
            H.assert_bits(read(db), b, kind, "max", "batch `in` untouched")


def peer_inputs(kind, n, P, seed):
    return [H.inputs(kind, n, seed=seed, peer=p) for p in range(P)]


@pytest.fixture(params=[0, 2], ids=["global_nt", "buffer_sc1"])
def fused_policy(request, device):
    """FMI_TUNE_FUSED_POLICY at the global and the buffer form, restored afterwards."""
    old = fmi_amd.tune_get(Tune.FUSED_POLICY)
    fmi_amd.tune_set(Tune.FUSED_POLICY, request.param)
    yield request.param
    fmi_amd.tune_set(Tune.FUSED_POLICY, old)


@pytest.mark.parametrize("P", [2, 3, 5, 8, 13, 16])
@pytest.mark.parametrize("kind", H.KINDS)
def test_fused_allreduce_every_rank(fused_policy, kind, P):
    """Peers alternate the two sides of every edge pair, so +0 and -0 (and NaN and a number) meet at the same
    index on different peers: max keeps an operand's own bits, and a wrong operand order shows."""
    for op in ("sum", "max"):
        for n in FUSED_SIZES:
            xs = peer_inputs(kind, n, P, seed=11)
            want, _ = orc.allreduce(xs, H.combiner(op, kind))
            ins = [bucket(x, kind) for x in xs]
            out = Bucket(n, DT[kind])
            for r in range(P):
                fmi_amd.reduce_tree(OP[op], Alg.ALLREDUCE, out, ins, rank=r)
                fmi_amd.sync()
                H.assert_bits(read(out), want[r], kind, op, f"{kind} {op} allreduce P={P} n={n} rank {r}")
            if op == "max" and n >= 8:
                assert any(not np.array_equal(want[0], want[r]) for r in range(1, P)), "ranks must differ on ±0"


@pytest.mark.parametrize("P", [3, 8, 16])
@pytest.mark.parametrize("kind", H.KINDS)
def test_fused_reduce_roots(fused_policy, kind, P):
    for op in ("sum", "max"):
        for n in FUSED_SIZES:
            xs = peer_inputs(kind, n, P, seed=12)
            ins = [bucket(x, kind) for x in xs]
            for root in (0, P - 1):
                want, _ = orc.reduce(xs, H.combiner(op, kind), root=root)
                out = Bucket(n, DT[kind])
                fmi_amd.reduce_tree(OP[op], Alg.REDUCE, out, ins, rank=root)
                fmi_amd.sync()
                H.assert_bits(read(out), want, kind, op, f"{kind} {op} reduce P={P} n={n} root {root}")


@pytest.mark.parametrize("P", [2, 3, 8, 16])
@pytest.mark.parametrize("kind", H.KINDS)
def test_fused_scan_every_output(fused_policy, kind, P):
    for op in ("sum", "max"):
        for n in FUSED_SIZES:
            xs = peer_inputs(kind, n, P, seed=13)
            want, _ = orc.scan(xs, H.combiner(op, kind))
            ins = [bucket(x, kind) for x in xs]
            outs = [Bucket(n, DT[kind]) for _ in range(P)]
            fmi_amd.scan_peers(OP[op], Alg.SCAN, outs, ins)
            fmi_amd.sync()
            for r in range(P):
                H.assert_bits(read(outs[r]), want[r], kind, op, f"{kind} {op} scan P={P} n={n} output {r}")
                H.assert_bits(read(ins[r]), xs[r], kind, "max", "scan input untouched")


def test_stepwise_forms_stay_exact(device):
    """The forms without a fused 16-bit float kernel run as pairwise passes in the same order: P = 17, and the
    left-to-right algorithms."""
    kind, op, n = "bf16", "sum", 2061
    f = H.combiner(op, kind)
    xs = peer_inputs(kind, n, 17, seed=14)
    ins = [bucket(x, kind) for x in xs]
    want, _ = orc.allreduce(xs, f)
    out = Bucket(n, DT[kind])
    for r in (0, 1, 16):
        fmi_amd.reduce_tree(Op.SUM, Alg.ALLREDUCE, out, ins, rank=r)
        fmi_amd.sync()
        H.assert_bits(read(out), want[r], kind, op, f"allreduce P=17 rank {r}")
    want, _ = orc.scan(xs, f)
    outs = [Bucket(n, DT[kind]) for _ in range(17)]
    fmi_amd.scan_peers(Op.SUM, Alg.SCAN, outs, ins)
    fmi_amd.sync()
    for r in range(17):
        H.assert_bits(read(outs[r]), want[r], kind, op, f"scan P=17 output {r}")
    xs, ins = xs[:5], ins[:5]
    want, _ = orc.reduce(xs, f, root=0, commutative=False, associative=False)
    fmi_amd.reduce_tree(Op.SUM, Alg.REDUCE_LTR, out, ins)
    fmi_amd.sync()
    H.assert_bits(read(out), want, kind, op, "reduce_ltr P=5")
    want, _ = orc.scan(xs, f, commutative=False, associative=False)
    fmi_amd.scan_peers(Op.SUM, Alg.SCAN_LTR, outs[:5], ins)
    fmi_amd.sync()
    for r in range(5):
        H.assert_bits(read(outs[r]), want[r], kind, op, f"scan_ltr P=5 output {r}")


@pytest.mark.parametrize("N", [2, 4])
@pytest.mark.parametrize("kind,op", [("bf16", "sum"), ("f16", "max")])
def test_comm_allreduce_tree_local(device, N, kind, op):
    """fmi_comm_allreduce, path TREE, LOCAL transport (ranks are threads on this GPU); n = 4 * 2048 + 5 so the shard
    padding runs. Every rank ends with the oracle simulation's value for that rank (max: ±0 ties differ by rank)."""
    from tests.test_gpu_comm import run_ranks

    n = 4 * 2048 + 5
    xs = peer_inputs(kind, n, N, seed=15)

    def body(c, r):
        s, out = bucket(xs[r], kind), Bucket(n, DT[kind])
        c.allreduce(OP[op], s, out, path=Path.TREE)
        fmi_amd.sync()
        return read(out), read(s)

    res = run_ranks(N, body)
    want, _ = orc.allreduce(xs, H.combiner(op, kind))
    for r in range(N):
        H.assert_bits(res[r][0], want[r], kind, op, f"comm allreduce {kind} {op} N={N} rank {r}")
        H.assert_bits(res[r][1], xs[r], kind, "max", "send bucket untouched")
    if op == "max":
        assert any(not np.array_equal(want[0], want[r]) for r in range(1, N))


@pytest.mark.parametrize("kind", H.KINDS)
def test_comm_rccl_path_single_rank(device, kind):
    """Path RCCL has a reduction type for the two dtypes: a one-rank communicator running the full exchange
    (ncclReduceScatter against itself) returns the input instead of FMI_ERR_UNSUPPORTED."""
    n = 4099
    x = H.inputs(kind, n, seed=16, peer=0)
    c = Comm(unique_id(Transport.RCCL), 1, 0, timeout_s=120)
    fmi_amd.tune_set(Tune.COMM_ONE_RANK_EXCHANGE, 1)
    try:
        s, out = bucket(x, kind), Bucket(x.size, DT[kind])
        c.allreduce(Op.SUM, s, out, path=Path.RCCL)
        c.sync()
        H.assert_bits(read(out), x, kind, "sum", f"path RCCL one rank {kind}")
    finally:
        fmi_amd.tune_set(Tune.COMM_ONE_RANK_EXCHANGE, 0)
        c.destroy()


@pytest.mark.parametrize("kind", H.KINDS)
def test_fill_synthetic(device, kind):
    n = 4099
    b = Bucket(n, DT[kind]).fill_synthetic(seed=42, peer=3)
    fmi_amd.sync()
    assert np.array_equal(read(b), H.synthetic(kind, n, seed=42, peer=3))
    b = Bucket(n, DT[kind]).fill_synthetic(seed=42, peer=3, first=1 << 33)
    fmi_amd.sync()
    assert np.array_equal(read(b), H.synthetic(kind, n, seed=42, peer=3, start=1 << 33))


def test_torch_glue_pair_combine(device):
    """fmi_amd.collectives on torch.bfloat16 / torch.float16 device tensors (a child process: torch must be loaded
    before the library) equals torch CPU's a + b on the same bits."""
    r = subprocess.run([sys.executable, "-u", "-m", "tests._half_torch_worker"], cwd=ROOT, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0 and "half torch glue ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_cpp_half_types_gpu(device):
    """Data<Dev::Bucket<Dev::bfloat16>> through FMI::Communicator: 3-peer allreduce (sum) and scan (max) equal the
    program's own host-path results bit for bit (fmi_amd/cpp/tests/test_half.cpp)."""
    exe = os.path.join(ROOT, "build", "cpp", "test_half")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fmi_amd", "cpp")], check=True)
    out = subprocess.run([exe, "--gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    assert "0 failed checks" in out.stderr
