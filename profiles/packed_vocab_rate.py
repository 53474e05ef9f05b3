"""The vocabulary ends of a packed model (K23) beside their dense forms, at Llama-3's [128256, 4096]: one JSON line per
(type, op, T).
  lm_head  ops.gemv_packed(q_type, blocks, x)        against F.linear(x, W), W the decoded bf16 weight, at T = 1 and 16
  embed    ops.embed_packed(q_type, blocks, ids)     against F.embedding(ids, W),                        at T = 1 and 2048
for Q4_K and Q6_K (Llama-3 files store output as Q6_K and token_embd as Q4_K or Q6_K), bf16, and the device bytes of both forms.
One process, HIP events, warm-up first, the candidates ALTERNATING, median of N with min-max, clocks as found; a measurement
is M = 8 back-to-back calls between two events, divided by M.  Cold weights: every candidate ROTATES through distinct copies
of its weight, at least 512 MiB of them between two uses of the same copy, so each lm_head call streams its weight from HBM
as a decode step that walked the whole model does (an embedding lookup touches T rows of a copy only).  Each round is
enqueued behind a matrix product of a few milliseconds, so the events bracket device time.  GB/s is algorithmic: the
weight's bytes plus x plus y over the median time.  The weight is an RTN-quantized 0.02 N(0, 1) matrix; x is N(0, 1).
usage: python profiles/packed_vocab_rate.py [N=15] [--out FILE]   (GPU box; needs only the built tree).  Writes FILE (default
profiles/packed_vocab_rate.txt) and prints the same lines."""
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from gptq_gguf_toolkit_amd import ops  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdecimal() else 15
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "packed_vocab_rate.txt")
DT = torch.bfloat16
NAMES = {12: "Q4_K", 14: "Q6_K"}
RING_BYTES = 512 << 20
M = 8
V, C = 128256, 4096


def ring(t):
    """Distinct copies of t: RING_BYTES of them and one more."""
    n = -(-RING_BYTES // (t.numel() * t.element_size())) + 1
    return [t] + [t.clone() for _ in range(n - 1)]


def measure(cands, blocker):
    """cands: {name: fn(i)}, i the call's number (it picks the copy of the weight)."""
    keys, calls = list(cands), 0
    for k in keys:
        for _ in range(2):
            cands[k](calls)
            calls += 1
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for it in range(N):
        evs = []
        blocker()
        for k in keys[it % len(keys):] + keys[:it % len(keys)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(M):
                cands[k](calls)
                calls += 1
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
    big = torch.randn(16384, 8192, device="cuda", generator=g).to(DT)
    blocker = lambda: torch.mm(big, big[:8192])  # noqa: E731
    W = torch.randn(V, C, device="cuda", generator=g) * 0.02
    for t in (12, 14):
        blocks = ops.pack(t, *ops.rtn_quantize(W, t))
        packed, dense = ring(blocks), ring(ops.dequantize_blocks(t, blocks, DT))
        head = {"type": NAMES[t], "V": V, "C": C, "dtype": "bf16", "packed_MB": round(blocks.numel() / 1e6, 1),
                "dense_MB": round(dense[0].numel() * 2 / 1e6, 1), "copies": len(packed), "dense_copies": len(dense), "launches": N * M}
        for T in (1, 16):
            x = torch.randn(T, C, device="cuda", generator=g).to(DT)
            m = measure({"packed": lambda i: ops.gemv_packed(t, packed[i % len(packed)], x),
                         "dense": lambda i: F.linear(x, dense[i % len(dense)])}, blocker)
            nbytes = blocks.numel() + 2 * T * (V + C)
            lines.append(json.dumps(dict(head, op="lm_head", T=T, packed=us(m["packed"]), dense=us(m["dense"]),
                                         packed_GBs=round(nbytes / m["packed"][0] / 1e9),
                                         dense_GBs=round((dense[0].numel() * 2 + 2 * T * (V + C)) / m["dense"][0] / 1e9),
                                         packed_over_dense=round(m["packed"][0] / m["dense"][0], 2))))
            print(lines[-1], flush=True)
        for T in (1, 2048):
            ids = torch.randint(0, V, (T,), device="cuda", generator=g)
            m = measure({"packed": lambda i: ops.embed_packed(t, packed[i % len(packed)], ids, DT),
                         "dense": lambda i: F.embedding(ids, dense[i % len(dense)])}, blocker)
            lines.append(json.dumps(dict(head, op="embed", T=T, packed=us(m["packed"]), dense=us(m["dense"]),
                                         packed_over_dense=round(m["packed"][0] / m["dense"][0], 2))))
            print(lines[-1], flush=True)
        del blocks, packed, dense
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
