#!/bin/bash
# GPU iteration for the 4-actor variant: its tests, then the whole GPU suite, then bench lines for TT and T4
set -o pipefail
export OUT="${OUT:-out}"      # results directory (relative to the repository root)
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 600 python -m pytest tests/test_t4_fused.py -m gpu -x -q -p no:cacheprovider > $OUT/pytest_t4.log 2>&1
rc=$?; tail -5 $OUT/pytest_t4.log; [ $rc -ne 0 ] && { tail -60 $OUT/pytest_t4.log; exit $rc; }
timeout -k 10 900 python -m pytest tests -m gpu -x -q -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1
rc=$?; tail -5 $OUT/pytest_gpu.log; [ $rc -ne 0 ] && { tail -60 $OUT/pytest_gpu.log; exit $rc; }
for v in TT T4; do
  for n in 16384 8192; do
    timeout -k 10 300 python bench.py --full --steps 2000 --warmup 200 --no-cpu-baseline --variant $v --num-envs $n > $OUT/bench_$v_$n.json 2> $OUT/bench.err || { tail -20 $OUT/bench.err; exit 1; }
    python - "$v" "$n" $OUT/bench_$v_$n.json <<'PY'
import json, sys
d=json.load(open(sys.argv[3]))
print("%s n=%s value %.1f M env-steps/s  kernel %.2f us  frac %.4f" % (sys.argv[1], sys.argv[2], d["value"]/1e6, d["roofline"]["avg_kernel_us"], d["roofline"]["frac"]))
PY
  done
done
