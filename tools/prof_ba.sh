#!/bin/bash
# GPU box: rocprofv3 kernel trace of the BA probe workload (diagnostic)
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
TAG=${1:-x}
OUT=${OUT:-bench_out}; mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python3 bench.py --steps 20 --warmup 3 --full --no-cpu > $OUT/prof_bench_$TAG.json 2> $OUT/prof_$TAG.err || { tail -30 $OUT/prof_$TAG.err; exit 1; }
