#!/bin/bash
# Build container: ablation libraries of the group step kernel (-DFJSP_GABLATE=n, fjsp_group.hip g_step) into .diag/:
# 1 state in / state out | 2 + update_parameter + task_select | 3 + machine_select | 4 + dispatch + event loop |
# 5 + second update_parameter + integer statistics + reward (no observation) | (0 = the product library)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $ROOT/.diag
for l in ${LEVELS:-1 2 3 4 5}; do
  (cd $ROOT && python3 -c "from deep_reinforcement_learning_for_fjsp_amd import _build
_build.build_library(force=True, out='.diag/libfjsp_gablate$l.so', defines=['FJSP_GABLATE=$l'])") &
done
wait
