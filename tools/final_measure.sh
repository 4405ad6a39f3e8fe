#!/bin/bash
# usage (on an MI355X, from the repo root): bash tools/final_measure.sh <tag>      e.g. r04_g
# the measurement set a round's records come from: full bench line, replayed-step kernel stats, MFMA / VALU busy pass,
# cfg3 per-kernel traffic (three rocprofv3 passes), the other configs, the GEMM table.  Everything lands in $OUT_DIR
# (default prof_out/); tools/collect_profiles.sh copies the judged files to profiles/.
t=$1
export OUT_DIR=${OUT_DIR:-prof_out}; mkdir -p "$OUT_DIR"; export OUT_DIR=$(cd "$OUT_DIR" && pwd)
python bench.py --full > $OUT_DIR/${t}_bench.json 2> $OUT_DIR/${t}_bench.err || exit 1
bash tools/prof.sh ${t} --full --no-lightpath --no-reference-scale --no-cpu-baseline > $OUT_DIR/${t}_prof.txt || exit 1
bash tools/pmc_multi.sh ${t}_pmc "GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_VALU" > /dev/null || exit 1
bash tools/pmc_all.sh ${t}_cfg3 tools/bench_configs.py cfg3 > $OUT_DIR/${t}_cfg3_pmc.txt || exit 1
python tools/bench_configs.py > $OUT_DIR/${t}_other_configs.jsonl 2>/dev/null || exit 1
python tools/bench_gemm.py > $OUT_DIR/${t}_gemm.jsonl || exit 1
echo ALLOK
