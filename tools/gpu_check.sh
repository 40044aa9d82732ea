# Full check of a tree on a GPU machine: the CPU suite (pytest -m "not gpu", run here too so a red contract test
# cannot slip past a GPU-only sequence), pytest -m gpu, smoke(), the plain bench.py line and the --full line.
# Usage (from the repo root): bash tools/gpu_check.sh        logs go to $OUT (default: run_out/)
set -o pipefail
OUT=${OUT:-run_out}
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest tests -m "not gpu" -x -q --timeout 300 > "$OUT/full_cpu.log" 2>&1 &&
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > "$OUT/full_gpu.log" 2>&1 &&
timeout -k 10 300 python -u -c 'import __graft_entry__ as g; g.smoke(); print("smoke ok")' > "$OUT/smoke.log" 2>&1 &&
timeout -k 10 200 python -u bench.py > "$OUT/bench.log" 2>&1 &&
timeout -k 10 600 python -u bench.py --full > "$OUT/bench_full.log" 2>&1
