"""The packed-weight decode (K22, gq_gemv_packed) beside the tile kernel and the dense Linear: one JSON line per (type, shape, T).
  gemv     ops.gemv_packed(q_type, blocks, x)                   -- K22
  tile     ops.linear_packed(q_type, blocks, x) at the same T   -- K21, the only packed forward before K22: the yardstick
  dense    F.linear(x, W), W the decoded dense weight           -- the forward of a dense-resident Linear (the vendor GEMM)
for each of Q2_K .. Q6_K, Q8_0, IQ4_NL and IQ4_XS at [R, C] in {4096 x 4096, 1024 x 4096, 14336 x 4096, 4096 x 14336} and T in {1, 2, 4, 8, 16},
bf16.  One process, HIP events, warm-up first, the candidates ALTERNATING (every candidate takes every place in the order),
median of N with min-max, clocks as found.  A measurement is M = 8 back-to-back calls of one candidate between two events,
divided by M: a pair of events around ONE launch of ten microseconds reads several microseconds too long, and back to back
is how a decode step issues its Linears (the figure includes the boundary between two dependent launches).
Cold weights: a [4096, 4096] Q4_K weight is 9.4 MB and even a bf16 one fits the 256 MiB last-level cache, so every candidate
ROTATES through distinct copies of its weight, at least 512 MiB of them between two uses of the same copy (the two packed
candidates share one ring and go on where the other stopped): each timed call reads its weight from HBM, as a decode step
that walks a whole model does.  x (at most 458 KB) is the same buffer every call, as the activations of a decode step are cache-hot.
Short kernels: launches of a few microseconds would be timed as the host's enqueue, so each round is enqueued behind a
matrix product of a few milliseconds that keeps the device busy meanwhile; the events then bracket device time alone.
GB/s is algorithmic: the weight's bytes plus x plus y over the median time.
Weights are RTN-quantized 0.02 N(0, 1) matrices (finite decodes), for the two IQ4 types, which have no encoder here, random
blocks with a small d (profiles/iq4_blocks.py); x is N(0, 1).
usage: python profiles/qgemv_rate.py [N=15] [--out FILE] [--types Q4_K,Q6_K] [--tokens 1,16] [--append]   (GPU box; needs only
the built tree; the two filters are for kernel A/B runs with GQ_SO_PATH and for adding types).  Writes FILE (default
profiles/qgemv_rate.txt; --append adds the run's lines to it) and prints the same lines; the last line names the largest T at which the GEMV was no slower than the
tile kernel in every row."""
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

N = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdecimal() else 15
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "qgemv_rate.txt")
DT = torch.bfloat16
NAMES = {10: "Q2_K", 11: "Q3_K", 12: "Q4_K", 13: "Q5_K", 14: "Q6_K", 8: "Q8_0", 20: "IQ4_NL", 23: "IQ4_XS"}
RING_BYTES = 512 << 20
M = 8
TS = tuple(int(v) for v in sys.argv[sys.argv.index("--tokens") + 1].split(",")) if "--tokens" in sys.argv else (1, 2, 4, 8, 16)
TYPES = sys.argv[sys.argv.index("--types") + 1].split(",") if "--types" in sys.argv else list(NAMES.values())


def ring(t):
    """Distinct copies of t, RING_BYTES of them and one more (and no fewer than two measurements' calls)."""
    n = max(-(-RING_BYTES // (t.numel() * t.element_size())) + 1, 2 * M)
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
    lines, worst = [], {T: 0.0 for T in TS}
    g = torch.Generator(device="cuda").manual_seed(0)
    big = torch.randn(16384, 8192, device="cuda", generator=g).to(DT)
    blocker = lambda: torch.mm(big, big[:8192])  # noqa: E731
    for R, C in ((4096, 4096), (1024, 4096), (14336, 4096), (4096, 14336)):
        W = torch.randn(R, C, device="cuda", generator=g) * 0.02
        for t in NAMES:
            if NAMES[t] not in TYPES:
                continue
            blocks = (iq4_blocks(t, R, C, g) if t in (20, 23) else ops.quantize_q8_0(W) if t == 8
                      else ops.pack(t, *ops.rtn_quantize(W, t)))
            packed, dense = ring(blocks), ring(ops.dequantize_blocks(t, blocks, DT))
            for T in TS:
                x = torch.randn(T, C, device="cuda", generator=g).to(DT)
                m = measure({"gemv": lambda i: ops.gemv_packed(t, packed[i % len(packed)], x),
                             "tile": lambda i: ops.linear_packed(t, packed[i % len(packed)], x),
                             "dense": lambda i: F.linear(x, dense[i % len(dense)])}, blocker)
                nbytes = blocks.numel() + 2 * T * (R + C)
                row = {"type": NAMES[t], "R": R, "C": C, "T": T, "dtype": "bf16", "launches": N * M, "weight_MB": round(blocks.numel() / 1e6, 1),
                       "copies": len(packed), "dense_copies": len(dense),
                       "gemv": us(m["gemv"]), "tile": us(m["tile"]), "dense": us(m["dense"]),
                       "gemv_GBs": round(nbytes / m["gemv"][0] / 1e9), "gemv_over_tile": round(m["gemv"][0] / m["tile"][0], 3),
                       "gemv_over_dense": round(m["gemv"][0] / m["dense"][0], 2)}
                worst[T] = max(worst[T], m["gemv"][0] / m["tile"][0])
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
                del x
            del blocks, packed, dense
        del W
    ok = [T for T in TS if all(worst[u] <= 1.0 for u in TS if u <= T)]
    lines.append(json.dumps({"worst_gemv_over_tile_by_T": {str(T): round(v, 3) for T, v in worst.items()},
                             "largest_T_gemv_no_slower_in_every_row": max(ok) if ok else 0}))
    print(lines[-1], flush=True)
    with open(OUT, "a" if "--append" in sys.argv else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
