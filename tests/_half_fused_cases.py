"""The (family, P, rank / root) cases of tests/test_gpu_half_fused.py, shared with tests/test_half_fused_cpu.py,
which pins the library's program at each of them to the oracle's symbolic expression."""

LTR_P = [2, 5, 16, 17, 31, 33, 128, 130, 255]  # fused; 17..31; the one-pass chain; segments with a carry-in
REDUCE_P = [17, 31, 100, 128, 129, 300]
ALLREDUCE_P = [17, 24, 31, 32, 64, 48, 80, 33, 100, 128]
SCAN_P = [17, 31, 32, 48, 100, 143, 144]
# further P the GPU file runs outside the four tables: both modes of FMI_TUNE_BLOCKS_ONE_PASS, the policy test,
# the communicator tests and the captured graph
EXTRA = {"allreduce": [20], "allreduce_ltr": [4], "scan": [33, 64], "scan_ltr": [4, 32], "reduce": [3, 8, 40], "ltr": []}

extra_ops_at = {"ltr": 5, "reduce": 31, "allreduce": 24, "scan": 31}  # the one P per family that also runs prod / min


def reduce_roots(P):
    return [0, 5, P - 1]


def allreduce_ranks(op, P):
    """sum: 0, 1, P - 1; max / min: also both sides of the 16-peer block edge."""
    ranks = [0, 1, P - 1] if op in ("sum", "prod") else [0, 1, 15, 16, 17, P - 1]
    return sorted({r for r in ranks if r < P})
