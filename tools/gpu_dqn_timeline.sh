#!/bin/bash
# On the GPU box: build the -DSGK_LEARN_TIMELINE variant of the library next to the product's and print dqn_sgd_kernel's
# barrier-to-barrier timeline (lane 0's wall_clock64 behind every barrier). Usage: tools/gpu_dqn_timeline.sh [out.log]
set -e
cd "$(dirname "$0")/.."
out=${1:-gpurun_out/dqn_timeline.log}
mkdir -p "$(dirname "$out")"
make -s -j6 -C safe-grid-agents_amd/csrc OUT=../lib/libsgk_tl.so OBJDIR=build_tl EXTRA="-DSGK_LEARN_TIMELINE"
: > "$out"
SGK_LIB_PATH=$PWD/safe-grid-agents_amd/lib/libsgk_tl.so SGK_NO_BUILD=1 python tools/exp_dqn_timeline.py 2>&1 | grep -v amdgpu.ids | tee -a "$out"
SGK_DQN_ONE_LAUNCH=1 SGK_LIB_PATH=$PWD/safe-grid-agents_amd/lib/libsgk_tl.so SGK_NO_BUILD=1 python tools/exp_dqn_timeline.py 2>&1 | grep -v amdgpu.ids | tee -a "$out"
