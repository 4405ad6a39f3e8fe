#!/bin/bash
# usage (from the repo root): bash tools/collect_profiles.sh <tag>   (after tools/final_measure.sh <tag>; records in $OUT_DIR, default prof_out/)
t=$1
O=${OUT_DIR:-prof_out}
cp $O/${t}_bench.json profiles/${t}_bench.json
cp $(ls $O/${t}/*/*kernel_stats.csv | head -1) profiles/${t}_graph_step_kernel_stats.csv
cp $O/${t}_pmc.json profiles/${t}_pmc_mfma_valu_counters.json
python tools/busy_from_pmc.py $O/${t}_pmc.json profiles/${t}_pmc_mfma_valu_busy.json > /dev/null
cp $O/${t}_cfg3_traffic.json profiles/r04_cfg3_traffic.json      # the file bench.py --full reads
cp $O/${t}_cfg3_kernel_stats.csv profiles/r04_cfg3_kernel_stats.csv
cp $O/${t}_other_configs.jsonl profiles/${t}_other_configs.jsonl
cp $O/${t}_gemm.jsonl profiles/${t}_gemm.jsonl
ls -la profiles/${t}_*
