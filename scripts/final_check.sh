#!/bin/bash
# Round-end GPU check (one call): pytest -m gpu, __graft_entry__.smoke(), and the bench with
# the driver's own flags (--steps 20 --warmup 5) plus --full; logs under $LOGS/final_*
# (default bench_logs/).
set -u
cd "$(dirname "$0")/.."; LOGS=${LOGS:-bench_logs}; mkdir -p $LOGS
timeout -k 10 900 python -u -m pytest -x -q --timeout 300 --timeout-method thread tests -m gpu > $LOGS/final_gpu_tests.log 2>&1; rc=$?; tail -3 $LOGS/final_gpu_tests.log; [ $rc = 0 ] || exit 1
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $LOGS/final_smoke.log 2>&1 || { tail -5 $LOGS/final_smoke.log; exit 1; }
tail -2 $LOGS/final_smoke.log
timeout -k 10 400 python bench.py --full --steps 20 --warmup 5 > $LOGS/final_bench_driver_flags.log 2>&1 || exit 1
grep '^{' $LOGS/final_bench_driver_flags.log | cut -c1-400
