"""The packed-weight forward (K21, gq_linear_packed) beside what dense residency pays: one JSON line per (type, shape, T).
One process, HIP events around each launch, warm-up first, the candidates ALTERNATING (every candidate takes every place in the
order), median of N with min-max, clocks as found.
  packed   ops.linear_packed(q_type, blocks, x)                 -- the forward of a packed-resident Linear
  dense    F.linear(x, W), W the decoded dense weight           -- the forward of a dense-resident Linear (the vendor GEMM)
  switch   ops.level_switch of that Linear (blocks -> W)        -- what a dense-resident search pays once per changed Linear
for each of Q2_K .. Q6_K, Q8_0, IQ4_NL and IQ4_XS at [R, C] in {4096 x 4096, 14336 x 4096, 4096 x 14336} and T in {2048, 8192},
bf16.  Weights are RTN-quantized 0.02 N(0, 1) matrices (finite decodes), for the two IQ4 types, which have no encoder here,
random blocks with a small d (profiles/iq4_blocks.py); x is N(0, 1).
usage: python profiles/qgemm_rate.py [N=9] [--out FILE] [--types Q4_K,IQ4_XS] [--append]   (GPU box; needs only the built tree).
Writes FILE (default profiles/qgemm_rate.txt; --append adds the run's lines to it) and prints the same lines."""
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from gptq_gguf_toolkit_amd import ops  # noqa: E402
from iq4_blocks import iq4_blocks  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdecimal() else 9
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "qgemm_rate.txt")
DT = torch.bfloat16
NAMES = {10: "Q2_K", 11: "Q3_K", 12: "Q4_K", 13: "Q5_K", 14: "Q6_K", 8: "Q8_0", 20: "IQ4_NL", 23: "IQ4_XS"}
TYPES = sys.argv[sys.argv.index("--types") + 1].split(",") if "--types" in sys.argv else list(NAMES.values())


def measure(cands):
    for fn in cands.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times, keys = {k: [] for k in cands}, list(cands)
    for it in range(N):
        evs = []
        for k in keys[it % len(keys):] + keys[:it % len(keys)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cands[k]()
            e1.record()
            evs.append((k, e0, e1))
        torch.cuda.synchronize()
        for k, e0, e1 in evs:
            times[k].append(e0.elapsed_time(e1) * 1e-3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def us(t3):
    return {"us": round(t3[0] * 1e6, 1), "min_us": round(t3[1] * 1e6, 1), "max_us": round(t3[2] * 1e6, 1)}


def main():
    lines = []
    g = torch.Generator(device="cuda").manual_seed(0)
    for R, C in ((4096, 4096), (14336, 4096), (4096, 14336)):
        W = torch.randn(R, C, device="cuda", generator=g) * 0.02
        for t in NAMES:
            if NAMES[t] not in TYPES:
                continue
            blocks = (iq4_blocks(t, R, C, g) if t in (20, 23) else ops.quantize_q8_0(W) if t == 8
                      else ops.pack(t, *ops.rtn_quantize(W, t)))
            Wd = ops.dequantize_blocks(t, blocks, DT)
            live = torch.empty_like(Wd)
            for T in (2048, 8192):
                x = torch.randn(T, C, device="cuda", generator=g).to(DT)
                m = measure({"packed": lambda: ops.linear_packed(t, blocks, x), "dense": lambda: F.linear(x, Wd),
                             "switch": lambda: ops.level_switch([(blocks, live, t, None)])})
                flops = 2.0 * T * R * C
                row = {"type": NAMES[t], "R": R, "C": C, "T": T, "dtype": "bf16", "launches": N,
                       "packed": us(m["packed"]), "dense": us(m["dense"]), "switch": us(m["switch"]),
                       "packed_TFLOPs": round(flops / m["packed"][0] / 1e12, 1), "dense_TFLOPs": round(flops / m["dense"][0] / 1e12, 1),
                       "packed_over_dense": round(m["packed"][0] / m["dense"][0], 2)}
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
                del x
            del blocks, Wd, live
        del W
    with open(OUT, "a" if "--append" in sys.argv else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
