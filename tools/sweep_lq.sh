#!/bin/bash
# usage (on the GPU box): bash tools/sweep_lq.sh -- lanes per key in the fix-up (H2_TUNE_LF = log2 F) at m = 3 .. 6 columns of 2^16,
# with a prebuilt tuning library variants/lib_tune.so (H2_BUILD_TUNING=1); one MSM launch sequence per step
cd "$GRAFT_REPO_ROOT"
cp halo2_prover_amd/libh2hip.so /tmp/libh2hip_keep.so
cp variants/lib_tune.so halo2_prover_amd/libh2hip.so
for m in 3 4 5 6; do
for lf in 2 3 4; do
  H2_TUNE_LF=$lf python3 bench.py --workload msm --msm-cols $m --steps 20 --warmup 3 --no-cpu-baseline --no-proof --no-extras 2>/dev/null | python3 -c '
import json,sys
d=json.loads(sys.stdin.read()); print("m='$m' LF='$lf' launch sequence: ms %.4f median %.4f" % (d["ms_per_step"], d["ms_per_step_median"]))'
done
done
cp /tmp/libh2hip_keep.so halo2_prover_amd/libh2hip.so
