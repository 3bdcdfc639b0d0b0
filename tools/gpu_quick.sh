set -eo pipefail
O=${PLBA_OUT:-bench_out}   # output directory
mkdir -p $O
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/gpu_tests_q.log 2>&1 || { tail -40 $O/gpu_tests_q.log; exit 1; }
tail -2 $O/gpu_tests_q.log
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/bench_q.json
python -c "import json;d=json.load(open('$O/bench_q.json'));print(d['value'],d['config']['ms_per_lm_iteration']);[print(k,v['us_per_launch']) for k,v in d['kernels'].items()]"
