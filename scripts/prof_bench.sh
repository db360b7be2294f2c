#!/bin/bash
# rocprofv3 kernel-trace stats of a short bench run -> bench_out/prof (or $RDN_OUT_ROOT/prof)
cd "$(dirname "$0")/.."; D=${RDN_OUT_ROOT:-bench_out}; mkdir -p $D; export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $D/prof -o run --output-format csv -- python3 bench.py --full --no-cpu-baseline --no-traffic --steps 10 --warmup 3 "$@" > $D/prof_bench.json 2> $D/prof.err
