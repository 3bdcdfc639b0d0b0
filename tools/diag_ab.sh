# Timing experiments (wrong results): bench per-kernel times under several PLBA_DIAG masks.
# Usage: tools/diag_ab.sh "0 1 2 4"
set -eo pipefail
O=${PLBA_OUT:-bench_out}   # output directory
mkdir -p $O
for v in $1; do
  PLBA_DIAG=$v timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/bench_diag.json 2> $O/bench_diag.err || true
  python -c "import json;d=json.load(open('$O/bench_diag.json'));print('[diag $v]', round(d['value'],1), {k: v['us_per_launch'] for k,v in d['kernels'].items()})" || tail -3 $O/bench_diag.err
done
