set -eo pipefail
O=${PLBA_OUT:-bench_out}   # output directory
export TMPDIR=/tmp
mkdir -p $O
timeout -k 10 300 python bench.py --full > $O/bench_r02f.json 2> $O/bench_r02f.err
cat $O/bench_r02f.json
timeout -k 10 300 python bench.py --full --config C5 --steps 10 > $O/bench_r02f_C5.json 2> $O/bench_r02f_C5.err
bash tools/profile_round.sh r02f C3
bash tools/profile_round.sh r02f C5 5
