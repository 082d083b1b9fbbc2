#!/bin/bash
# Build container: the ablation libraries of tools/ablate_step.py (-DFJSP_ABLATE=n) into .diag/ so that the GPU box's
# minutes go to measuring, not compiling (tools/ablate_pmc_prebuilt.sh reads them there).  .diag/ is git-ignored and
# listed in .gpurunignore: remove its line there for the one gpurun call that needs the libraries.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
LEVELS=${LEVELS:-"1 2 3 4 7 8 9"}
mkdir -p $ROOT/.diag
for l in $LEVELS; do
  (cd $ROOT && python3 -c "from deep_reinforcement_learning_for_fjsp_amd import _build
_build.build_library(force=True, out='.diag/libfjsp_ablate$l.so', defines=['FJSP_ABLATE=$l'])") &
done
wait
ls -la $ROOT/.diag/
