#!/bin/bash
# GPU box: smoke, 1-GPU bench, rocprofv3 kernel-trace summary of the same command, and two
# separate PMC passes (FETCH_SIZE, WRITE_SIZE) for roofline.traffic.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}; mkdir -p $OUT
export TMPDIR=/tmp
TAG=${1:-r01}
STEPS=${2:-50}
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { cat $OUT/smoke.log; exit 1; }
tail -1 $OUT/smoke.log
timeout -k 10 600 python bench.py --steps $STEPS --warmup 5 --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -30 $OUT/bench_$TAG.err; exit 1; }
cat $OUT/bench_$TAG.json
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python3 bench.py --steps 20 --warmup 3 --full --no-cpu > $OUT/prof_bench_$TAG.json 2> $OUT/prof_$TAG.err || { tail -30 $OUT/prof_$TAG.err; exit 1; }
for C in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 600 rocprofv3 --pmc $C --kernel-trace -d $OUT/pmc_${TAG}_$C -o run --output-format csv -- python3 bench.py --steps 10 --warmup 2 --no-cpu --no-rows --pipeline-frames 0 > $OUT/pmc_bench_${TAG}_$C.json 2> $OUT/pmc_${TAG}_$C.err || { tail -30 $OUT/pmc_${TAG}_$C.err; exit 1; }
done
find $OUT/prof_$TAG $OUT/pmc_${TAG}_* -name "*.csv" | head -20
python tools/pmc_summary.py $OUT/pmc_${TAG} $OUT/pmc_traffic_${TAG}.json
python tools/kstats.py $OUT/prof_$TAG > $OUT/kstats_$TAG.txt
# keep the summaries; the raw per-dispatch traces run to tens of MiB
rm -f $OUT/prof_$TAG/run_kernel_trace.csv $OUT/pmc_${TAG}_*/run_counter_collection.csv $OUT/pmc_${TAG}_*/run_kernel_trace.csv
du -sh $OUT
