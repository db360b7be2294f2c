#!/bin/bash
# B16 + B32 train-step lines with per-layer reports (OUT=dir under bench_out/, or under $RDN_OUT_ROOT); no tests
cd "$(dirname "$0")/.."; D=${RDN_OUT_ROOT:-bench_out}/${OUT:-base}; mkdir -p $D; export TMPDIR=/tmp
for b in 16 32; do
  timeout -k 10 200 python bench.py --full --batch $b --no-extra --no-cpu-baseline --no-inference --no-traffic --steps 30 --warmup 5 --layer-report $D/b${b}.layers.json > $D/b${b}.json 2>$D/b${b}.err || exit $?
done
