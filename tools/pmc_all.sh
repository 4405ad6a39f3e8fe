#!/bin/bash
# usage: tools/pmc_all.sh <tag> <python script + args, relative to the repo root>
# three rocprofv3 runs of the same command (FETCH_SIZE pass, WRITE_SIZE pass, kernel trace + stats) -> $OUT_DIR/<tag>_*
tag=$1; shift
R=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)      # the repository root
OUT=${OUT_DIR:-$R/prof_out}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)   # where the records land (OUT_DIR, default prof_out/)
cd /tmp && export TMPDIR=/tmp
for ctr in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $ctr --kernel-trace --output-format csv -d $OUT/${tag}_$ctr -- python3 $R/$1 "${@:2}" > $OUT/${tag}_$ctr.log 2>&1 || exit 1
done
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${tag}_stats -- python3 $R/$1 "${@:2}" > $OUT/${tag}_stats.log 2>&1 || exit 1
F=$(ls $OUT/${tag}_FETCH_SIZE/*/*counter_collection.csv | head -1)
W=$(ls $OUT/${tag}_WRITE_SIZE/*/*counter_collection.csv | head -1)
S=$(ls $OUT/${tag}_stats/*/*kernel_stats.csv | head -1)
cp $S $OUT/${tag}_kernel_stats.csv
python3 $R/tools/traffic_table.py $F $W $S $OUT/${tag}_traffic.json "command: $*"
