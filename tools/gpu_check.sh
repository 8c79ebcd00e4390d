#!/bin/bash
# One GPU-box pass: parity tests, smoke, bench. Each GPU step has its own time
# limit; a crash/timeout/fault exit code stops the script (no retries).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
LOGS=${LOGS:-bench_out}  # where the logs go
mkdir -p $LOGS
STEPS=${STEPS:-64}
timeout -k 10 600 python tools/gemv_sweep.py ${SWEEP_MODES:-auto tasks} > $LOGS/sweep.log 2>&1; rc=$?; echo "sweep rc=$rc"; cat $LOGS/sweep.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 900 python -m pytest tests -m gpu -q -p no:cacheprovider ${PYTEST_ARGS:-} > $LOGS/gpu_tests.log 2>&1
rc=$?
echo "pytest rc=$rc"; tail -25 $LOGS/gpu_tests.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as e; e.smoke()" > $LOGS/smoke.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -3 $LOGS/smoke.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 600 python bench.py --full --steps "$STEPS" --warmup 8 --cpu-seconds 8 ${BENCH_ARGS:-} > $LOGS/bench.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -3 $LOGS/bench.log
exit $rc
