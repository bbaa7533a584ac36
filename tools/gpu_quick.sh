#!/bin/bash
# quick GPU iteration: parity tests + bench line
set -o pipefail
export OUT="${OUT:-out}"      # results directory (relative to the repository root)
mkdir -p $OUT
timeout -k 10 900 python -m pytest tests -m gpu -x -q -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1
rc=$?; tail -5 $OUT/pytest_gpu.log; [ $rc -ne 0 ] && { tail -40 $OUT/pytest_gpu.log; exit $rc; }
timeout -k 10 600 python bench.py --full --steps 2000 --warmup 200 --no-cpu-baseline ${BENCH_ARGS} > $OUT/bench_quick.json 2> $OUT/bench.err || { tail -20 $OUT/bench.err; exit 1; }
python - <<'PY'
import os
import json
d=json.load(open(os.environ["OUT"] + "/bench_quick.json"))
print("value %.1f M env-steps/s  kernel %.2f us  frac %.4f" % (d["value"]/1e6, d["roofline"]["avg_kernel_us"], d["roofline"]["frac"]))
PY
