set -x
OUT=${OUT:?set OUT to the output directory}
mkdir -p $OUT
python bench.py --steps 10 --warmup 3 --full --no-cpu-baseline --no-whole-model --no-side-legs 2>$OUT/base_bench.err | tail -1 > $OUT/base_bench_compact.json
cat $OUT/base_bench_compact.json
GQ_PROF_DUMP=$OUT/tl_base.txt python bench.py --steps 3 --warmup 2 --full --breakdown --no-cpu-baseline --no-whole-model --no-side-legs 2>$OUT/base_breakdown.err | tail -1
python profiles/timeline.py $OUT/tl_base.txt > $OUT/timeline_base.txt 2>&1; head -60 $OUT/timeline_base.txt
bash profiles/trace_chain.sh > $OUT/trace_chain_base.txt 2>&1; cat $OUT/trace_chain_base.txt
bash profiles/r06_syrk_pmc.sh
