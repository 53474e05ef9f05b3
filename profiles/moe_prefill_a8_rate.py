"""One whole expert FFN of a packed MoE layer's grouped PREFILL on int8 activations against the two things it could replace: one
JSON line per (type, T).
  q8   PackedExperts.forward with prefill = "grouped", act = "q8"  -- K36: gq_moe_route, ONE gq_quantize_act_q8 shared by the gate and
                                                                     up launch of gq_linear_packed_experts_a8,
                                                                     gq_silu_mul_quantize_act_q8, the down launch, the combine
  fp   the same module with act = "fp"                            -- K25's grouped path (gq_linear_packed_experts), unchanged by K36
  hf   transformers' MixtralExperts.forward (its own loop)        -- on the decoded bf16 weights, host synchronisations included
and, on their own, the two quantizer launches of a q8 call (quant: gq_quantize_act_q8 of the [T, H] hidden states; fused:
gq_silu_mul_quantize_act_q8 of the [T * K, I] gate / up, as one launch over all pairs), and max_memory_allocated above what is
resident before the call for both act values.
Shapes, routing, method (one process, HIP events, warm-up, candidates alternating behind a blocker, median of N with min-max, cold
weights through COPIES layers) are profiles/moe_prefill_rate.py's, whose functions this script runs.
usage: python profiles/moe_prefill_a8_rate.py [N=7] [--out FILE]   (GPU box; needs only the built tree).
Writes FILE (default profiles/moe_prefill_a8_rate.txt) and prints the same lines; the last line names the points where q8 lost."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import moe_prefill_rate as base  # noqa: E402  (puts the tree on sys.path; reads N from the command line)
import torch  # noqa: E402
from gptq_gguf_toolkit_amd import ops  # noqa: E402
from gptq_gguf_toolkit_amd.packed_experts import ROLES, PackedExperts  # noqa: E402

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "moe_prefill_a8_rate.txt")
E, K, H, I, DT, COPIES = base.E, base.K, base.H, base.I, base.DT, base.COPIES


def peak_above_resident(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn(0)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


@torch.no_grad()
def main():
    lines, lost = [], []
    g = torch.Generator(device="cuda").manual_seed(0)
    big = torch.randn(16384, 8192, device="cuda", generator=g).to(DT)
    blocker = lambda: torch.mm(big, big[:8192])  # noqa: E731
    hf, hf_loop = base.hf_experts()
    for t in base.NAMES:
        layers, dense = [], []
        for c in range(COPIES):
            mod = PackedExperts(E, H, I, DT)
            mod.prefill = "grouped"
            for role in ROLES:
                R, C = mod.role_shape(role)
                W = torch.randn(E * R, C, device="cuda", generator=g) * 0.02
                mod.set_level(role, ops.pack(t, *ops.rtn_quantize(W, t)).view(-1), t)
                del W
            layers.append(mod)
            dense.append((mod.dense_gate_up(), mod.dense_weight("down")))
        for T in base.TS:
            x = torch.randn(T, H, device="cuda", generator=g).to(DT)
            w, idx = torch.topk(torch.rand(T, E, device="cuda", generator=g), K, -1)  # uniformly random distinct experts
            w = w / w.sum(-1, keepdim=True)
            counts = torch.bincount(idx.reshape(-1), minlength=E).tolist()
            gu = [torch.randn(T * K, I, device="cuda", generator=g).to(DT) for _ in range(2)]

            def run(act):
                def call(i):
                    mod = layers[i % COPIES]
                    mod.act = act
                    return mod(x, idx, w)
                return call

            def hf_call(i):
                hf.gate_up_proj, hf.down_proj = dense[i % COPIES]
                return hf_loop(hf, x, idx, w)

            assert layers[0].takes_prefill_path(T, K) and PackedExperts.act == "fp"
            layers[0].act = "q8"
            assert layers[0].takes_q8_path(T, K)
            m = base.measure({"q8": run("q8"), "fp": run("fp"), "hf": hf_call, "quant": lambda i: ops.quantize_act_q8(x),
                              "fused": lambda i: ops.silu_mul_quantize_act_q8(*gu)}, blocker)
            flop = 2.0 * T * K * 3 * I * H
            row = {"type": base.NAMES[t], "E": E, "K": K, "H": H, "I": I, "T": T, "dtype": "bf16", "pairs_per_expert": counts,
                   "chunks": -(-T * K // PackedExperts.prefill_max_pairs), "calls": base.N * base.M, "copies": COPIES}
            for k in m:
                row[k] = base.us(m[k])
            for k in ("q8", "fp", "hf"):
                row[k + "_TFLOPs"] = round(flop / m[k][0] / 1e12, 1)
            row["q8_over_fp"] = round(m["q8"][0] / m["fp"][0], 3)
            row["q8_over_hf"] = round(m["q8"][0] / m["hf"][0], 3)
            row["peak_bytes_above_resident"] = {a: peak_above_resident(run(a)) for a in ("q8", "fp")}
            lost += [(base.NAMES[t], T, k) for k in ("fp", "hf") if m["q8"][0] > m[k][0]]
            del gu
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
        hf.gate_up_proj = hf.down_proj = None
        del layers, dense
        torch.cuda.empty_cache()
    lines.append(json.dumps({"q8_no_slower_at_every_point": not lost, "points_lost": lost, "act_default": PackedExperts.act}))
    print(lines[-1], flush=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
