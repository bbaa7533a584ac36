#!/bin/bash
# Runs on the GPU box (via gpurun): GPU parity tests, smoke, bench, rocprofv3 kernel trace.
set -o pipefail
export OUT="${OUT:-out}"      # results directory (relative to the repository root)
mkdir -p $OUT
export TMPDIR=/tmp
echo "== pytest -m gpu" | tee $OUT/progress.log
timeout -k 10 900 python -m pytest tests -m gpu -x -q -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1
rc=$?; tail -25 $OUT/pytest_gpu.log; echo "pytest rc=$rc" | tee -a $OUT/progress.log
[ $rc -ne 0 ] && exit $rc
echo "== smoke" | tee -a $OUT/progress.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tee $OUT/smoke.log || exit 1
echo "== bench" | tee -a $OUT/progress.log
timeout -k 10 600 python bench.py --full --steps 2000 --warmup 200 > $OUT/bench.json 2> $OUT/bench.err || { tail -20 $OUT/bench.err; exit 1; }
cat $OUT/bench.json
echo "== rocprofv3 kernel trace" | tee -a $OUT/progress.log
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python bench.py --full --steps 2000 --warmup 200 --no-cpu-baseline --no-configs > $OUT/bench_prof.json 2> $OUT/prof.err || { tail -20 $OUT/prof.err; exit 1; }
cat $OUT/bench_prof.json
find $OUT/prof -name "*stats*" | head; for f in $(find $OUT/prof -name "*kernel_stats.csv"); do head -12 $f; done
