# A/B of two libbnn builds on one box: ab/libbnn_a.so (A) against the in-tree library (B),
# alternating default-bench runs (kernel timers on), ROUNDS rounds.  bash tools/gpu_ab.sh [rounds]
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}   # logs and profiles land here (git-ignored)
cd $R && mkdir -p $OUT
for r in $(seq 1 ${1:-2}); do
  for v in A B; do
    if [ $v = A ]; then export BNN_LIB=$R/ab/libbnn_a.so; else unset BNN_LIB; fi
    timeout -k 10 300 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-gpu-torch ${BENCH_ARGS} > $OUT/ab_$v$r.log 2>&1 || { echo "RUN $v$r FAIL"; tail -5 $OUT/ab_$v$r.log; exit 1; }
    tail -1 $OUT/ab_$v$r.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); k=d['kernels']; print('$v$r', d['ms_per_step'], ' '.join(f'{n[:14]}={v[\"avg_us\"]:.0f}' for n,v in list(k.items())[:7]))"
  done
done
