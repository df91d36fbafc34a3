#!/bin/bash
# BASELINE configs 2-4 on one GPU (bench.py --full --config N), one line each in $OUT/config<N>.txt
# (OUT defaults to bench_out/ in the repository root)
set -o pipefail
cd ${GRAFT_REPO_ROOT:-.}
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 400 python bench.py --full --config 2 --steps 2 --warmup 1 --no-cpu-baseline --no-frame-setup --heavy-frame -1 --animation 0 > $OUT/config2.txt 2>&1 || exit $?
timeout -k 10 500 python bench.py --full --config 3 --steps 1 --warmup 1 --no-cpu-baseline --no-frame-setup --heavy-frame -1 > $OUT/config3.txt 2>&1 || exit $?
timeout -k 10 600 python bench.py --full --config 4 --steps 1 --warmup 0 --no-cpu-baseline --no-frame-setup > $OUT/config4.txt 2>&1 || exit $?
echo done
