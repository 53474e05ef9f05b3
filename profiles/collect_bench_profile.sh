#!/bin/bash
# The judged artifacts of a round: the bench line and the rocprofv3 --kernel-trace --stats summary of the same
# command.  usage (GPU box): OUT=<dir> bash profiles/collect_bench_profile.sh r02   -> $OUT/<tag>_bench_line.json,
# $OUT/<tag>_bench_kernel_stats.csv (copy both into profiles/).
R=${GRAFT_REPO_ROOT:-/root/repo}; TAG=${1:-r02}
OUT=${OUT:?set OUT to the output directory}
cd $R && python bench.py --steps 5 --warmup 2 --full 2>$OUT/${TAG}_bench.err | tail -1 > $OUT/${TAG}_bench_line.json
cd /tmp && export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o p -- python $R/bench.py --steps 5 --warmup 2 --no-cpu-baseline --no-whole-model --no-side-legs > $OUT/${TAG}_prof.log 2>&1 || echo "rocprofv3 failed"
cp $(find $OUT/${TAG}_prof -name "*kernel_stats.csv" | head -1) $OUT/${TAG}_bench_kernel_stats.csv
tail -1 $OUT/${TAG}_prof.log | cut -c1-300
head -12 $OUT/${TAG}_bench_kernel_stats.csv | cut -c1-160
