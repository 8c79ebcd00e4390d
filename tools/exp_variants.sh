set -u
cd "${GRAFT_REPO_ROOT}"
LOGS=${LOGS:-bench_out}  # where the logs go
mkdir -p $LOGS
V=ggml-neon-opt_amd/lib/variants
timeout -k 10 600 python tools/gemv_sweep.py auto lib=$V/libw8.so lib=$V/libw16.so lib=$V/libw12d4.so > $LOGS/sweep5.log 2>&1 || exit $?
for L in "" $V/libw8.so $V/libw16.so $V/libw12d4.so; do
  if [ -n "$L" ]; then export MI355X_LIB=$PWD/$L; else unset MI355X_LIB; fi
  echo "lib=${L:-default}" >> $LOGS/bench5.log
  timeout -k 10 300 python bench.py --full --steps 64 --warmup 8 --no-cpu-baseline --no-large 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['value'], d['ms_per_step'], d['kernels'])" >> $LOGS/bench5.log || exit $?
done
cat $LOGS/sweep5.log $LOGS/bench5.log
