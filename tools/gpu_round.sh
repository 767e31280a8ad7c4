#!/bin/bash
# One GPU round on a gpurun box: parity tests, smoke, bench, rocprofv3 evidence (summaries: tools/summarize_prof.py).
#   OUT=<results folder> bash tools/gpu_round.sh [noprof]     (bench.py runs with --full: every figure of the round)
# Every GPU step has a time limit of its own; the first step that fails, faults or times out ends the script.
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-build/round}
mkdir -p "$OUT"
timeout -k 10 1500 python -m pytest tests -m gpu -q -s > "$OUT/pytest_gpu.log" 2>&1; rc=$?; echo "pytest rc=$rc" >> "$OUT/pytest_gpu.log"
tail -4 "$OUT/pytest_gpu.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1; rc=$?; echo "smoke rc=$rc" >> "$OUT/smoke.log"; tail -2 "$OUT/smoke.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 900 python bench.py --full > "$OUT/bench.log" 2>&1 || exit $?
tail -1 "$OUT/bench.log" > "$OUT/bench_latest.json"; cut -c1-400 "$OUT/bench_latest.json"
timeout -k 10 600 python tools/gpu_diag.py > "$OUT/stage_cycles.raw" 2>&1 || exit $?
grep -v amdgpu.ids "$OUT/stage_cycles.raw" > "$OUT/stage_cycles.txt"; tail -3 "$OUT/stage_cycles.txt" | cut -c1-200
if [ "$1" != "noprof" ]; then timeout -k 10 3000 bash tools/gpu_profile.sh > "$OUT/profile.log" 2>&1 || exit $?; tail -2 "$OUT/profile.log"; fi
