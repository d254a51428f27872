# Full GPU session: parity tests, smoke, bench (wide/mlp/cnn), rocprofv3 kernel-trace stats and
# separate PMC passes (FETCH_SIZE, WRITE_SIZE) of the default bench.  Every GPU step has its own
# time limit; the script stops at the first failure.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}   # logs and profiles land here (git-ignored)
TAG=${TAG:-r01}
cd $R
mkdir -p $OUT
timeout -k 10 400 python -u -m pytest tests/ -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/parity_$TAG.log 2>&1 || { echo PARITY FAIL; tail -30 $OUT/parity_$TAG.log; exit 1; }
tail -1 $OUT/parity_$TAG.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1 || { echo SMOKE FAIL; tail -20 $OUT/smoke_$TAG.log; exit 1; }
tail -1 $OUT/smoke_$TAG.log
timeout -k 10 400 python bench.py --full > $OUT/bench_wide_$TAG.log 2>&1 || { echo BENCH FAIL; tail -30 $OUT/bench_wide_$TAG.log; exit 1; }
tail -1 $OUT/bench_wide_$TAG.log | cut -c1-400
timeout -k 10 300 python bench.py --full --config mlp --steps 20 --warmup 3 > $OUT/bench_mlp_$TAG.log 2>&1 || { echo BENCH MLP FAIL; tail -30 $OUT/bench_mlp_$TAG.log; exit 1; }
tail -1 $OUT/bench_mlp_$TAG.log | cut -c1-300
timeout -k 10 300 python bench.py --full --config cnn --steps 20 --warmup 3 --no-cpu-baseline > $OUT/bench_cnn_$TAG.log 2>&1 || { echo BENCH CNN FAIL; tail -30 $OUT/bench_cnn_$TAG.log; exit 1; }
tail -1 $OUT/bench_cnn_$TAG.log | cut -c1-300
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o wide --output-format csv -- python3 $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof_$TAG.log 2>&1 || { echo PROF FAIL; tail -20 $OUT/prof_$TAG.log; exit 1; }
tail -1 $OUT/prof_$TAG.log | cut -c1-300
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_cnn_$TAG -o cnn --output-format csv -- python3 $R/bench.py --full --config cnn --steps 10 --warmup 2 --no-cpu-baseline > $OUT/prof_cnn_$TAG.log 2>&1 || { echo PROF CNN FAIL; tail -20 $OUT/prof_cnn_$TAG.log; exit 1; }
timeout -s KILL 240 rocprofv3 --pmc FETCH_SIZE -d $OUT/pmc_fetch_$TAG -o wide --output-format csv -- python3 $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-kernel-timing > $OUT/pmc_fetch_$TAG.log 2>&1 || { echo PMC1 FAIL; tail -20 $OUT/pmc_fetch_$TAG.log; exit 1; }
timeout -s KILL 240 rocprofv3 --pmc WRITE_SIZE -d $OUT/pmc_write_$TAG -o wide --output-format csv -- python3 $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-kernel-timing > $OUT/pmc_write_$TAG.log 2>&1 || { echo PMC2 FAIL; tail -20 $OUT/pmc_write_$TAG.log; exit 1; }
find $OUT/prof_$TAG $OUT/pmc_fetch_$TAG $OUT/pmc_write_$TAG -name "*.csv"
