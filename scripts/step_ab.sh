#!/bin/bash
# one measurement round: GPU suite (minus the PSNR experiment), per-layer conv3_big vs conv3_halo, B16 + B32 step with layer reports (OUT=dir under bench_out/, or under $RDN_OUT_ROOT)
cd "$(dirname "$0")/.."; D=${RDN_OUT_ROOT:-bench_out}/${OUT:-step}; mkdir -p $D; export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests/ -k "not psnr" -m gpu -x -v -s --timeout 200 --timeout-method thread > $D/t.log 2>&1
rc=$?; echo "tests rc=$rc" >> $D/t.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python scripts/big_plans.py $D/plans.json > $D/plans.log 2>&1 || exit $?
for b in 16 32; do
  timeout -k 10 150 python bench.py --full --batch $b --no-extra --no-cpu-baseline --no-inference --no-traffic --steps 30 --warmup 5 --layer-report $D/b${b}.layers.json > $D/b${b}.json 2>/dev/null || exit $?
done
