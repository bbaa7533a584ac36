#!/bin/bash
# 27-dof evidence: bench line at BASELINE config 5's per-GPU size + rocprofv3 kernel trace of the same command
set -o pipefail
export OUT="${OUT:-out}"      # results directory (relative to the repository root)
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 600 python bench.py --full --variant TA --num-envs 4096 --steps 2000 --warmup 200 > $OUT/bench_TA.json 2> $OUT/bench_TA.err || { tail -20 $OUT/bench_TA.err; exit 1; }
cat $OUT/bench_TA.json
rm -rf $OUT/prof_TA
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_TA -- python bench.py --full --variant TA --num-envs 4096 --steps 2000 --warmup 200 --no-cpu-baseline > $OUT/bench_TA_prof.json 2> $OUT/prof_TA.err || { tail -20 $OUT/prof_TA.err; exit 1; }
for f in $(find $OUT/prof_TA -name "*kernel_stats.csv"); do head -4 $f | cut -c1-300; done
