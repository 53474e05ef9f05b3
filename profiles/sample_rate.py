"""The sampler (K23, gq_sample_logits) beside the torch expression of the same rule: one JSON line per (V, B, top_k, dtype).
  kernel   ops.sample_logits(logits, u, top_k, top_p, t)               -- one launch
  torch    topk -> / t -> softmax -> cumsum, nucleus mask, cumsum -> first j with cdf > u * total -> gather
           (the same rule on the same tensor with the same u; five-odd launches and a sort)
for V in {32000, 128256}, B in {1, 8}, top_k in {40, 1024}, fp16 and fp32 logits, top_p = 0.9, temperature = 0.8; logits are
3 N(0, 1).  One process, HIP events, warm-up first, the two candidates ALTERNATING, median of N with min-max, clocks as found.
A measurement is M = 8 back-to-back calls between two events, divided by M (a pair of events around one launch of ten
microseconds reads several microseconds too long).  The logits are the SAME buffer every call: in a decode step they were
written by the lm_head a moment ago and come from the caches, so a cold read is not what a sampler sees.  Each round is
enqueued behind a matrix product of a few milliseconds, so the events bracket device time, not the host's enqueue.  `agree` is
the fraction of rows on which the two return the same token (they differ in the exp and in the order of the fp32 sums).
usage: python profiles/sample_rate.py [N=15] [--out FILE]   (GPU box; needs only the built tree).  Writes FILE (default
profiles/sample_rate.txt) and prints the same lines."""
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402
from gptq_gguf_toolkit_amd import ops  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdecimal() else 15
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "sample_rate.txt")
M = 8
TOP_P, TEMP = 0.9, 0.8


def torch_chain(logits, u, top_k, top_p, t):
    v, idx = torch.topk(logits.float(), top_k, dim=-1)
    w = torch.softmax(v / t, -1)
    cdf = w.cumsum(-1)
    w = w * ((cdf - w) < top_p)  # the smallest n whose mass reaches top_p
    cdf = w.cumsum(-1)
    j = (cdf > u[:, None] * cdf[:, -1:]).int().argmax(-1)
    return idx.gather(-1, j[:, None]).squeeze(-1)


def measure(cands, blocker):
    keys = list(cands)
    for k in keys:
        for _ in range(2):
            cands[k]()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for it in range(N):
        evs = []
        blocker()
        for k in keys[it % len(keys):] + keys[:it % len(keys)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(M):
                cands[k]()
            e1.record()
            evs.append((k, e0, e1))
        torch.cuda.synchronize()
        for k, e0, e1 in evs:
            times[k].append(e0.elapsed_time(e1) * 1e-3 / M)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def us(t3):
    return {"us": round(t3[0] * 1e6, 1), "min_us": round(t3[1] * 1e6, 1), "max_us": round(t3[2] * 1e6, 1)}


def main():
    lines = []
    g = torch.Generator(device="cuda").manual_seed(0)
    big = torch.randn(16384, 8192, device="cuda", generator=g).to(torch.bfloat16)
    blocker = lambda: torch.mm(big, big[:8192])  # noqa: E731
    for V in (32000, 128256):
        for B in (1, 8):
            base = 3 * torch.randn(B, V, device="cuda", generator=g)
            u = torch.rand(B, device="cuda", generator=g)
            for dt, name in ((torch.float16, "f16"), (torch.float32, "f32")):
                logits = base.to(dt)
                for top_k in (40, 1024):
                    m = measure({"kernel": lambda: ops.sample_logits(logits, u, top_k, TOP_P, TEMP),
                                 "torch": lambda: torch_chain(logits, u, top_k, TOP_P, TEMP)}, blocker)
                    agree = float((ops.sample_logits(logits, u, top_k, TOP_P, TEMP) == torch_chain(logits, u, top_k, TOP_P, TEMP)).float().mean())
                    greedy = measure({"kernel": lambda: ops.sample_logits(logits, None, top_k, TOP_P, 0.0),
                                      "torch": lambda: logits.argmax(-1)}, blocker)
                    row = {"V": V, "B": B, "top_k": top_k, "dtype": name, "top_p": TOP_P, "temperature": TEMP, "launches": N * M,
                           "kernel": us(m["kernel"]), "torch": us(m["torch"]),
                           "kernel_over_torch": round(m["kernel"][0] / m["torch"][0], 3), "agree": agree,
                           "argmax_kernel": us(greedy["kernel"]), "argmax_torch": us(greedy["torch"])}
                    lines.append(json.dumps(row))
                    print(lines[-1], flush=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
