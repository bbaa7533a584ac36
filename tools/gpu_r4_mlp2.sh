#!/bin/bash
set -o pipefail
export OUT="${OUT:-out}"      # results directory (relative to the repository root)
mkdir -p $OUT; export TMPDIR=/tmp
timeout -k 10 600 python -m pytest tests/test_policy_mlp.py tests/test_policy_backward.py -m gpu -x -q -p no:cacheprovider > $OUT/pytest_mlp.log 2>&1 || { tail -30 $OUT/pytest_mlp.log; exit 1; }
tail -3 $OUT/pytest_mlp.log
timeout -k 10 300 python tools/gpu_mlp_layers.py 4096 313 2>&1 | grep -v "amdgpu.ids\|fused" | cut -c1-72 | tee $OUT/mlp_layers_4096.txt || exit 1
timeout -k 10 300 python tools/rollout_bench.py --variant TA --num-envs 4096 --policy native > $OUT/rollout_TA_native.json 2> $OUT/rollout.err || { tail -20 $OUT/rollout.err; exit 1; }
cut -c1-700 $OUT/rollout_TA_native.json
