"""The packed decode step on int8 activations (K37, gq_gemv_packed_a8) beside the 16-bit GEMV and the dense Linear: one JSON line
per (type, shape, T).
  a8       ops.gemv_packed_q8(q_type, blocks, x)   -- K37: ONE launch, the activation quantizer inside
  gemv     ops.gemv_packed(q_type, blocks, x)      -- K22, the decode path without the flag: the yardstick, in the same run
  dense    F.linear(x, W), W the decoded weight    -- the forward of a dense-resident Linear (the vendor GEMM)
for each of Q2_K .. Q6_K and Q8_0 at [R, C] in {4096 x 4096, 1024 x 4096, 14336 x 4096, 4096 x 14336} and T in {1, 4}, bf16.
The method is profiles/qgemv_rate.py's and its `measure` is imported from there: one process, HIP events around M = 8
back-to-back calls behind a blocker, the candidates alternating, median of N with min-max, every candidate rotating through
at least 512 MiB of distinct copies of its weight (the two packed candidates share one ring), x cache-hot.  GB/s is
algorithmic: the weight's bytes plus x plus y over the median time.  `diff` is max |a8 - gemv| / max |gemv| on the timed
operands: the two differ by the 8-bit quantization of x, nothing larger.
usage: python profiles/qgemv_a8_rate.py [N=15] [--out FILE]   (GPU box; needs only the built tree).  Writes FILE (default
profiles/qgemv_a8_rate.txt) and prints the same lines."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
out_arg = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
import qgemv_rate as base  # noqa: E402  (reads N from sys.argv; its --out default is not used here)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from gptq_gguf_toolkit_amd import ops  # noqa: E402

OUT = out_arg or os.path.join(HERE, "qgemv_a8_rate.txt")
NAMES = {t: base.NAMES[t] for t in (10, 11, 12, 13, 14, 8)}
TS = (1, 4)


def main():
    lines = []
    g = torch.Generator(device="cuda").manual_seed(0)
    big = torch.randn(16384, 8192, device="cuda", generator=g).to(base.DT)
    blocker = lambda: torch.mm(big, big[:8192])  # noqa: E731
    for R, C in ((4096, 4096), (1024, 4096), (14336, 4096), (4096, 14336)):
        W = torch.randn(R, C, device="cuda", generator=g) * 0.02
        for t in NAMES:
            blocks = ops.quantize_q8_0(W) if t == 8 else ops.pack(t, *ops.rtn_quantize(W, t))
            packed, dense = base.ring(blocks), base.ring(ops.dequantize_blocks(t, blocks, base.DT))
            for T in TS:
                x = torch.randn(T, C, device="cuda", generator=g).to(base.DT)
                ya, yg = ops.gemv_packed_q8(t, blocks, x).float(), ops.gemv_packed(t, blocks, x).float()
                m = base.measure({"a8": lambda i: ops.gemv_packed_q8(t, packed[i % len(packed)], x),
                                  "gemv": lambda i: ops.gemv_packed(t, packed[i % len(packed)], x),
                                  "dense": lambda i: F.linear(x, dense[i % len(dense)])}, blocker)
                nbytes = blocks.numel() + 2 * T * (R + C)
                row = {"type": NAMES[t], "R": R, "C": C, "T": T, "dtype": "bf16", "launches": base.N * base.M,
                       "weight_MB": round(blocks.numel() / 1e6, 1), "copies": len(packed), "dense_copies": len(dense),
                       "a8": base.us(m["a8"]), "gemv": base.us(m["gemv"]), "dense": base.us(m["dense"]),
                       "a8_GBs": round(nbytes / m["a8"][0] / 1e9), "a8_over_gemv": round(m["a8"][0] / m["gemv"][0], 3),
                       "a8_over_dense": round(m["a8"][0] / m["dense"][0], 2),
                       "diff": round(float((ya - yg).abs().max() / yg.abs().max()), 5)}
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
                del x
            del blocks, packed, dense
        del W
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
