#!/usr/bin/env python3
"""kernel_trace.csv -> counts / mean us of the kernels of interest over the last iteration, far-next durations in order."""
import csv, glob, sys
d = sys.argv[1]
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
rows = list(csv.DictReader(open(f)))
name = [k for k in rows[0] if k.lower() == "kernel_name"][0]
st = [k for k in rows[0] if k.lower().startswith("start")][0]
en = [k for k in rows[0] if k.lower().startswith("end")][0]
rows.sort(key=lambda r: int(r[st]))
# last iteration = from the last equil_kernel on
idx = max(i for i, r in enumerate(rows) if "equil_kernel" in r[name])
last = rows[idx:]
span = (max(int(r[en]) for r in last) - int(last[0][st])) / 1e6
print(f"last iteration: {len(last)} kernels, span {span:.2f} ms (from equil_kernel)")
agg = {}
for r in last:
    n = r[name]
    a = agg.setdefault(n, [0, 0.0]); a[0] += 1; a[1] += (int(r[en]) - int(r[st])) / 1e3
for n, (c, us) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
    print(f"{n[:90]:90s} {c:5d} {us/1e3:9.3f} ms {us/c:9.1f} us")
far = [(int(r[en]) - int(r[st])) / 1e3 for r in last if "gemm32_chain_full_kernel" in r[name]]
print("far-next launches in order (us):", " ".join(f"{x:.0f}" for x in far))
segs = [r for r in last if "gptq_segment_kernel" in r[name]]
if segs:
    t_first = int(segs[0][st]); t_last = max(int(r[en]) for r in last)
    print(f"column loop (first segment kernel -> last kernel): {(t_last - t_first)/1e6:.2f} ms")
    hp = (t_first - int(last[0][st])) / 1e6
    print(f"h_prepare (equil_kernel -> first segment kernel): {hp:.2f} ms")
