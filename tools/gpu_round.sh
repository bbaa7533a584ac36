#!/bin/bash
# The full evidence set of a build: GPU tests, smoke, bench line (with cpu_baseline), rocprofv3 kernel trace, PMC passes.
set -o pipefail
export OUT="${OUT:-out}"      # results directory (relative to the repository root)
bash tools/gpu_check.sh || exit 1
rm -rf $OUT/pmc; bash tools/gpu_pmc.sh || exit 1
