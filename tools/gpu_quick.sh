set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
LOGS=${LOGS:-bench_out}  # where the logs go
mkdir -p $LOGS
timeout -k 10 400 python -u -m pytest tests/test_gpu_mmf.py tests/test_gpu_ops.py tests/test_gpu_parity.py -x -q --timeout 200 --timeout-method thread -p no:cacheprovider > $LOGS/t1.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -15 $LOGS/t1.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 500 python -u bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-large --no-70b > $LOGS/b1.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -c 300 $LOGS/b1.log
exit $rc
