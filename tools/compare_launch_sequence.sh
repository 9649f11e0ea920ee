#!/bin/bash
# Kernel launch sequence of two builds of the library over tools/estep_launch_sequence.py: same kernels, same order, same grids?
#   tools/compare_launch_sequence.sh OLD/libprobreg_hip.so NEW/libprobreg_hip.so OUTDIR
# One traced process per build (kernel trace only, no counters), each under its own time limit; nothing starts after a failure.
set -euo pipefail
old_lib=$1 new_lib=$2 out=$3
cd "$(dirname "$0")/.."
mkdir -p "$out"
PROBREG_HIP_LIB=$old_lib timeout -k 10 420 rocprofv3 --kernel-trace -d "$out/old" -o t -- python tools/estep_launch_sequence.py > "$out/old.log" 2>&1 &&
PROBREG_HIP_LIB=$new_lib timeout -k 10 420 rocprofv3 --kernel-trace -d "$out/new" -o t -- python tools/estep_launch_sequence.py > "$out/new.log" 2>&1 &&
python tools/estep_launch_sequence.py --compare "$(find "$out/old" -name '*.db' | head -1)" "$(find "$out/new" -name '*.db' | head -1)" | tee "$out/compare.txt"
