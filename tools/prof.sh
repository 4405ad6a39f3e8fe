#!/bin/bash
# usage: tools/prof.sh <tag> [bench args...]   (kernel stats of one bench run -> $OUT_DIR/<tag>/, prints the top kernels)
tag=$1; shift
R=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)      # the repository root
OUT=${OUT_DIR:-$R/prof_out}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)   # where the records land (OUT_DIR, default prof_out/)
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$tag -- python3 $R/bench.py "$@" > $OUT/$tag.log 2>&1
python3 - <<PY
import csv,glob
f=glob.glob("$OUT/$tag/*/*kernel_stats.csv")[0]
rows=list(csv.DictReader(open(f)))
for r in rows[:28]:
    print(f"{r['Name'][:100]:100s} n={r['Calls']:>5s} tot_us={float(r['TotalDurationNs'])/1e3:9.1f} avg_us={float(r['AverageNs'])/1e3:8.1f} {float(r['Percentage']):5.1f}%")
PY
