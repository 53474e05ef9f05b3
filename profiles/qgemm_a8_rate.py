"""The packed forward on int8 activations (K35) beside the paths it stands next to: one JSON line per (type, shape, T).
The method is profiles/qgemm_rate.py's: one process, HIP events around each candidate, warm-up first, the candidates
ALTERNATING (every candidate takes every place in the order), median of N with min-max, clocks as found.
  q8       ops.linear_packed_q8(q_type, blocks, x)   -- quantizer + integer GEMM, what PackedLinear(act="q8") runs
  quant    ops.quantize_act_q8(x)                    -- the quantizer alone
  packed   ops.linear_packed(q_type, blocks, x)      -- the 16-bit packed forward (K21)
  dense    F.linear(x, W), W the decoded weight      -- the vendor GEMM of a dense-resident Linear
for each of Q2_K .. Q6_K and Q8_0 at [R, C] in {4096 x 4096, 14336 x 4096, 4096 x 14336} and T in {2048, 8192}, bf16.
usage: python profiles/qgemm_a8_rate.py [N=9] [--out FILE]   (GPU box; needs only the built tree).
Writes FILE (default profiles/qgemm_a8_rate.txt) and prints the same lines."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import qgemm_rate as base  # noqa: E402  (measure, us, N, DT: the same method)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from gptq_gguf_toolkit_amd import ops  # noqa: E402

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "qgemm_a8_rate.txt")
NAMES = {10: "Q2_K", 11: "Q3_K", 12: "Q4_K", 13: "Q5_K", 14: "Q6_K", 8: "Q8_0"}


def main():
    g = torch.Generator(device="cuda").manual_seed(0)
    with open(OUT, "w") as f:
        for R, C in ((4096, 4096), (14336, 4096), (4096, 14336)):
            W = torch.randn(R, C, device="cuda", generator=g) * 0.02
            for t in NAMES:
                blocks = ops.quantize_q8_0(W) if t == 8 else ops.pack(t, *ops.rtn_quantize(W, t))
                Wd = ops.dequantize_blocks(t, blocks, base.DT)
                for T in (2048, 8192):
                    x = torch.randn(T, C, device="cuda", generator=g).to(base.DT)
                    m = base.measure({"q8": lambda: ops.linear_packed_q8(t, blocks, x), "quant": lambda: ops.quantize_act_q8(x),
                                      "packed": lambda: ops.linear_packed(t, blocks, x), "dense": lambda: F.linear(x, Wd)})
                    row = {"type": NAMES[t], "R": R, "C": C, "T": T, "dtype": "bf16", "launches": base.N,
                           **{k: base.us(m[k]) for k in ("q8", "quant", "packed", "dense")},
                           "q8_TOPs": round(2.0 * T * R * C / m["q8"][0] / 1e12, 1),
                           "q8_over_packed": round(m["q8"][0] / m["packed"][0], 2), "q8_over_dense": round(m["q8"][0] / m["dense"][0], 2)}
                    line = json.dumps(row)
                    f.write(line + "\n")
                    f.flush()
                    print(line, flush=True)
                    del x
                del blocks, Wd
            del W


if __name__ == "__main__":
    main()
