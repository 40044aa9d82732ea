# C2 profiles for profiles/: kernel trace + stats of the default bench command with --full (C2, then C3 and C4 on
# one GPU), then separate --pmc FETCH_SIZE and --pmc WRITE_SIZE passes (MI355X_MICROARCH.md HBM recipe), then an
# unprofiled run for comparison. Output goes to $OUT (default: run_out/ under the repo root).
# Every profiled pass runs with --no-c5 --no-cpu-baseline: C5's host_pair_reduce block launches the same
# pair_tile<OpSum, float> instantiation on 1 GiB page-locked HOST buckets (PCIe-bound, ~40 ms a launch) and the
# CPU baseline's c1_reference GPU leg launches it on 1 MiB staged buckets; rocprofv3's per-name --stats average
# would mix those with C2's 256 MiB HBM launches (tools/pmc_summarize.py keeps shapes apart anyway).
set -e
R=$PWD
O=$(realpath -m "${OUT:-$R/run_out}")
W=$(mktemp -d)  # rocprofv3 writes its temporary files into the working directory: keep them out of the tree
trap 'rm -rf "$W"' EXIT
mkdir -p $O/c2t $O/c2f $O/c2w
cd $W
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/c2t -o run -- python3 $R/bench.py --full --no-c5 --no-cpu-baseline > $O/c2_bench_under_rocprof.txt 2> $O/c2t.err
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/c2f -o run -- python3 $R/bench.py --full --no-cpu-baseline --no-c5 --steps 40 --warmup 5 > $O/c2f.log 2>&1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/c2w -o run -- python3 $R/bench.py --full --no-cpu-baseline --no-c5 --steps 40 --warmup 5 > $O/c2w.log 2>&1
cd $R
timeout -k 10 200 python3 bench.py --full --no-cpu-baseline > $O/c2_bench_plain.json
