#!/bin/bash
# usage (on the GPU box): bash tools/pstats.sh <tag> [N]  -- rocprofv3 kernel stats of N Poseidon k=16 proofs through the C ABI (keygen every call)
cd "$GRAFT_REPO_ROOT" && export TMPDIR=/tmp
export OUT=${OUT:-out}; mkdir -p "$OUT"   # where the artefacts go (relative to the repository root)
tag=${1:-p}; N=${2:-10}
rm -rf $OUT/pprof_$tag
rocprofv3 --kernel-trace --stats -d $OUT/pprof_$tag -o run --output-format csv -- python3 tools/proof_profile.py $N > $OUT/${tag}_proof.txt 2> $OUT/${tag}_perr.txt
f=$(find $OUT/pprof_$tag -name '*kernel_stats.csv' | head -1)
python3 - "$f" $N > $OUT/${tag}_pstats.txt <<'P'
import csv,sys
N=int(sys.argv[2])+1
tot=0
for r in csv.DictReader(open(sys.argv[1])):
    t=float(r['TotalDurationNs'])/1000/N; tot+=t
    print(r['Name'][:64].ljust(64), ("%.1f"%(int(r['Calls'])/N)).rjust(6), ("%.1f"%(float(r['AverageNs'])/1000)).rjust(9), ("%.1f us/proof"%t).rjust(16))
print("total GPU us per proof (incl. one-time setup kernels / N): %.1f"%tot)
P
cp "$f" $OUT/${tag}_proof_kernel_stats.csv
rm -rf $OUT/pprof_$tag
head -24 $OUT/${tag}_pstats.txt; tail -1 $OUT/${tag}_pstats.txt; cat $OUT/${tag}_proof.txt
