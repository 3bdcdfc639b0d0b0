#!/bin/bash
# GPU-box round check: parity tests, smoke, default bench, rocprofv3 stats + PMC passes.
# Usage (from the repo root, on the GPU box): tools/gpu_round.sh <tag> [pytest -k expr]
set -eo pipefail
O=${PLBA_OUT:-bench_out}   # output directory
TAG=${1:-r01}
export TMPDIR=/tmp
mkdir -p $O
echo "[gpu_round] tests" >&2
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread \
    ${2:+-k "$2"} > $O/gpu_tests_${TAG}.log 2>&1
tail -3 $O/gpu_tests_${TAG}.log >&2
echo "[gpu_round] smoke" >&2
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke_${TAG}.log 2>&1
echo "[gpu_round] bench" >&2
timeout -k 10 400 python bench.py --full > $O/bench_${TAG}.json 2> $O/bench_${TAG}.err
cat $O/bench_${TAG}.json >&2
echo "[gpu_round] profile" >&2
bash tools/profile_bench.sh ${TAG} C3
echo "[gpu_round] done" >&2
