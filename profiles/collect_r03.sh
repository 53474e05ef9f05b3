#!/bin/bash
# Round-3 judged artifacts, one per BASELINE config that fits one GPU:
#   gpurun_out/r03/r03_bench_<workload>.json            the bench line (roofline, trailing_update, cpu_baseline)
#   gpurun_out/r03/r03_bench_<workload>_kernel_stats.csv  rocprofv3 --kernel-trace --stats of the same workload
#   gpurun_out/r03/r03_syrk_traffic.json + r03_syrk_fetch_dispatches.csv   rocprofv3 --pmc FETCH_SIZE pass (default workload)
# usage (GPU box): bash profiles/collect_r03.sh [workload ...]      then copy gpurun_out/r03/* into profiles/
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=$R/gpurun_out/r03
mkdir -p $OUT
WLS=${@:-"llama3-8b-block-q4k llama3-8b-block-mixed tinyllama-block-q4k llama3-70b-block-q4k mixtral-block"}
# L2-miss read bytes of the SYRK launches of the default bench command (its own pass: --pmc with --kernel-trace only)
cd /tmp && export TMPDIR=/tmp
timeout 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_fetch -o p -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-whole-model --no-side-legs > $OUT/pmc_fetch.log 2>&1 || echo "pmc pass failed"
python3 - <<PY
import csv, glob, hashlib, json, os
rows = []
for f in glob.glob("$OUT/pmc_fetch/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "syrk16" in r["Kernel_Name"] and r["Counter_Name"] == "FETCH_SIZE":
            rows.append((int(r["Dispatch_Id"]), int(r["Grid_Size"]), float(r["Counter_Value"])))
rows.sort()
with open("$OUT/r03_syrk_fetch_dispatches.csv", "w") as f:
    f.write("dispatch_id,grid_size,FETCH_SIZE,GB_corrected\n")
    for d, g, v in rows:
        f.write(f"{d},{g},{v:.6g},{v * 2048 / 1e9:.3f}\n")
if rows:
    per = sum(v for _, _, v in rows) * 2048 / 1e9 / len(rows)
    T, n4, n14 = 65536, 3, 1
    alg = (4 * (n4 * (T * 4096 * 2 + 2 * 4096 * 4096 * 4)) + 4 * (T * 14336 * 2 + 2 * 14336 * 14336 * 4)) / 8 / 1e9
    h = hashlib.sha256()
    for fn in sorted(glob.glob("$R/gptq-gguf-toolkit_amd/csrc/*.h*")):
        h.update(open(fn, "rb").read())
    json.dump({"GB_per_launch": round(per, 2), "algorithmic_GB_per_launch": round(alg, 2), "launches": len(rows),
               "kernel_sources_sha256": h.hexdigest()[:16],
               "measured_on": "rocprofv3 --pmc FETCH_SIZE x 2 KB (gfx950 correction) of bench.py --steps 2 --warmup 1, "
                              "default workload; per-dispatch values: profiles/r03_syrk_fetch_dispatches.csv"},
              open("$OUT/r03_syrk_traffic.json", "w"))
    print(f"{len(rows)} SYRK launches, {per:.2f} GB per launch (algorithmic {alg:.2f})")
PY
rm -rf $OUT/pmc_fetch
cp $OUT/r03_syrk_traffic.json $R/profiles/r03_syrk_traffic.json  # bench.py reads it (and checks the source hash)
for W in $WLS; do
  EXTRA=""
  [ "$W" != "llama3-8b-block-q4k" ] && EXTRA="--no-whole-model"
  cd $R && timeout 900 python bench.py --workload $W --steps 5 --warmup 2 --full $EXTRA 2>$OUT/r03_bench_$W.err | tail -1 > $OUT/r03_bench_$W.json
  (cd /tmp && export TMPDIR=/tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$W -o p -- \
     python $R/bench.py --workload $W --steps 5 --warmup 2 --no-cpu-baseline --no-whole-model --no-side-legs > $OUT/prof_$W.log 2>&1 || echo "rocprofv3 failed for $W")
  cp $(find $OUT/prof_$W -name "*kernel_stats.csv" | head -1) $OUT/r03_bench_${W}_kernel_stats.csv 2>/dev/null
  rm -rf $OUT/prof_$W
  python3 -c "
import json,sys
d=json.loads(open('$OUT/r03_bench_$W.json').read())
print('$W', d['ms_per_step'], 'ms/step', d['value'], 'Mparams/s  syrk frac', d['roofline']['frac'], ' trailing whole', (d.get('trailing_update') or {}).get('whole_alone',{}).get('frac'), ' cpu', (d.get('cpu_baseline') or {}).get('value'))
" 2>&1 | tail -1
done
