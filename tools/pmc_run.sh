#!/bin/bash
# usage (on the GPU box): bash tools/pmc_run.sh  -- the two PMC passes of the short bench + the stamped summary in $OUT/pmc_traffic.json
cd "$GRAFT_REPO_ROOT" && export TMPDIR=/tmp
export OUT=${OUT:-out}; mkdir -p "$OUT"   # where the artefacts go (relative to the repository root)
rm -rf $OUT/pmc_f $OUT/pmc_w
ARGS="--steps 3 --warmup 0 --full --no-cpu-baseline --no-proof --no-extras"
rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/pmc_f -o run --output-format csv -- python3 bench.py $ARGS > /dev/null 2> $OUT/pmc_f_err.txt || exit 1
rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/pmc_w -o run --output-format csv -- python3 bench.py $ARGS > /dev/null 2> $OUT/pmc_w_err.txt || exit 1
python3 tools/pmc_traffic.py $OUT/pmc_f $OUT/pmc_w $OUT/pmc_traffic.json 6 && python3 - $OUT/pmc_traffic.json <<'P'
import json, sys
d = json.load(open(sys.argv[1]))
for k, v in d.get("kernels", {}).items():
    print(k[:40].ljust(40), {a: (round(b) if isinstance(b, float) else b) for a, b in v.items()})
P
rm -rf $OUT/pmc_f $OUT/pmc_w
