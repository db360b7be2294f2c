#!/bin/bash
# quick GPU check: selected test files (TESTS), then B16 + B32 train-step lines with
# per-layer reports (OUT=dir under bench_out/, or under $RDN_OUT_ROOT).  Each step under its own limit.
cd "$(dirname "$0")/.."; D=${RDN_OUT_ROOT:-bench_out}/${OUT:-check}; mkdir -p $D; export TMPDIR=/tmp
if [ -n "$TESTS" ]; then
  timeout -k 10 600 python -u -m pytest $TESTS -m gpu -x -v --timeout 300 --timeout-method thread > $D/tests.log 2>&1
  rc=$?; echo "tests rc=$rc" >> $D/tests.log; [ $rc -eq 0 ] || exit $rc
fi
[ -n "$NO_BENCH" ] && exit 0
for b in ${BATCHES:-16 32}; do
  timeout -k 10 200 python bench.py --full --batch $b --no-extra --no-cpu-baseline --no-inference --no-traffic --steps 30 --warmup 5 --layer-report $D/b${b}.layers.json > $D/b${b}.json 2>$D/b${b}.err || exit $?
done
