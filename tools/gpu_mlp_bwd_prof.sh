#!/bin/bash
# Evidence for the policy backward at the learner's minibatch: per-layer times next to PyTorch / hipBLASLt, rocprofv3 kernel stats, PMC (matrix-core
# busy cycles, LDS bank conflicts of the transposed reads).  Run on the GPU box: bash tools/gpu_mlp_bwd_prof.sh [tag]
export OUT="${OUT:-out}"      # results directory (relative to the repository root)
tag=${1:-r03}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $OUT
timeout -k 10 300 python tools/gpu_mlp_bwd_layers.py 32768 313 > $OUT/${tag}_mlp_bwd_layers_32768.txt 2>&1 || { tail -5 $OUT/${tag}_mlp_bwd_layers_32768.txt; exit 1; }
cat $OUT/${tag}_mlp_bwd_layers_32768.txt
rm -rf $OUT/prof_bwd
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_bwd -- python tools/gpu_mlp_bwd_layers.py 32768 313 > $OUT/prof_bwd.log 2>&1 || { tail -5 $OUT/prof_bwd.log; exit 1; }
f=$(find $OUT/prof_bwd -name '*kernel_stats.csv' | head -1); cp $f $OUT/${tag}_mlp_bwd_kernel_stats.csv; head -12 $f
MLP_TOOL=tools/gpu_mlp_bwd_layers.py MLP_M=32768 MLP_K=313 bash tools/gpu_mlp_pmc.sh && cp $OUT/pmc_mlp/summary.csv $OUT/${tag}_mlp_bwd_pmc_summary.csv
