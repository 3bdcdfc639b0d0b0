#!/bin/bash
# GPU box, repo root: bench.py at one config under several environment settings, one line each.
# usage: tools/ab_env.sh <tag> <config> "<ENV=val ...>" ["<ENV=val ...>" ...]   ("-" = no extra env)
set -o pipefail
O=${PLBA_OUT:-bench_out}   # output directory
TAG=$1; CFG=$2; shift 2
mkdir -p $O
for rep in 1 2; do
for e in "$@"; do
  [ "$e" = "-" ] && e=""
  env $e timeout -k 10 120 python3 bench.py --full --config $CFG --steps 20 --warmup 3 --no-cpu-baseline --no-host-mirror --windows 0 \
      > $O/ab_${TAG}.json 2> $O/ab_${TAG}.err || { tail -5 $O/ab_${TAG}.err; exit 1; }
  python3 -c "
import json,sys
d=json.load(open('$O/ab_${TAG}.json'))
k=d['kernels']
print('%-28s %8.1f it/s steps %s fac %s  ' % ('$e' or 'default', d['value'], d['config']['speculative_trials'].get('device_steps_per_lba'), d['config']['factorisation']) + ' '.join('%s=%.1f' % (n[2:], v['us_per_launch']) for n, v in k.items()))
" | tee -a $O/ab_${TAG}.txt
done
done
