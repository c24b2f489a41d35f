set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${1:-profile_out}
mkdir -p $OUT/prof_v6 $OUT/pmc_v6
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_v6 -o run --output-format csv -- python3 bench.py --full --steps 20 --warmup 3 --cpu-seconds 0 > $OUT/prof_v6/bench_traced.json 2> $OUT/prof_v6/stderr.log || { echo TRACE_FAIL; tail -5 $OUT/prof_v6/stderr.log; exit 1; }
echo trace ok
bash tools/pmc_traffic.sh $OUT/pmc_v6 --steps 5 --warmup 1 --cpu-seconds 0 --no-extra || { echo PMC_FAIL; exit 1; }
echo pmc ok
python3 tools/traffic.py $OUT/pmc_v6 k_pooled_vec criteo26_b65536 $OUT/pmc_v6/traffic.json | tail -1
timeout -k 10 300 python3 bench.py --full > $OUT/bench_v6f.json 2> $OUT/bench_v6f.err || { echo BENCH_FAIL; exit 1; }
echo bench ok
