#!/bin/bash
# usage (on the GPU box): bash tools/pmc_calib.sh -- the two counter passes of tools/pmc_calib.hip -> $OUT/pmc_calibration.json
cd "$GRAFT_REPO_ROOT" && export TMPDIR=/tmp
export OUT=${OUT:-out}; mkdir -p "$OUT"   # where the artefacts go (relative to the repository root)
rm -rf $OUT/cal_f $OUT/cal_w
rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/cal_f -o run --output-format csv -- ./halo2_prover_amd/build/pmc_calib > $OUT/cal_req.json 2> $OUT/cal_f_err.txt || exit 1
rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/cal_w -o run --output-format csv -- ./halo2_prover_amd/build/pmc_calib > /dev/null 2> $OUT/cal_w_err.txt || exit 1
python3 tools/pmc_calib.py $OUT/cal_f $OUT/cal_w $OUT/cal_req.json $OUT/pmc_calibration.json
rm -rf $OUT/cal_f $OUT/cal_w
