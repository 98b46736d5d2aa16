#!/bin/bash
# One GPU call: rocprofv3 trace + PMC passes for every bench workload (--full: the traceback kernels
# are profiled too), then the default bench line with its CPU baseline.
# Usage: tools/profile_all.sh <tag> ; WORKLOADS overrides the list; output in $OUT_DIR (default bench_out/).
tag=${1:-run}
set -o pipefail
out=${OUT_DIR:-bench_out}
mkdir -p $out
for w in ${WORKLOADS:-headline batch local dna8k protein4k}; do
  bash tools/profile.sh ${tag}_$w --workload $w --full --no-cpu-baseline --steps 5 --warmup 1 || exit 1
done
timeout -k 10 300 python bench.py --full > $out/${tag}_bench_default.json 2> $out/${tag}_bench_default.err || exit 1
cat $out/${tag}_bench_default.json
