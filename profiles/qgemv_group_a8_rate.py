"""The grouped dense decode launches on int8 activations (K39, gq_gemv_packed_group_a8) beside the launches they replace: one
JSON line per (types, T, part), at Llama-3-8B's shapes (hidden 4096, q 4096 rows, k and v 1024, intermediate 14336), bf16.
  part qkv     group: ops.gemv_packed_group_q8 on (q, k, v), ONE launch          single: three ops.gemv_packed_q8
  part swiglu  group: ops.gemv_swiglu_packed_q8 on (gate, up), ONE launch        single: two ops.gemv_packed_q8 and ops.fwd_silu_mul
  part layer   group: qkv, o, gate-up-SwiGLU, down: FOUR launches                single: the EIGHT launches of decode_act="q8"
               (the Linears and SwiGLU only: no attention, norms or residuals; every launch on fixed inputs of its shape)
for types Q4_K, Q6_K and `mix` (q, k, gate, up Q4_K; v, o, down Q6_K -- the pairing a Q4_K_M file has; its swiglu part is
Q4_K's and is not repeated) and T in {1, 4}.
The method is profiles/qgemv_rate.py's and its `measure` is imported from there: one process, HIP events around M = 8
back-to-back calls behind a blocker, the candidates alternating, median of N with min-max; call i reads copy i % n of the
layer's weights, n copies so that the q / k / v of a pass over the ring alone exceed 512 MiB; x cache-hot.  `equal` is the bit
equality of the two candidates' outputs on the timed operands.
The last line is whole-model: generate.greedy on the tiny Llama of the tests (hidden 256, 2 layers, built and quantized here,
mixed K-quants) loaded --packed --decode_act q8 with and without --decode_group on, 64 new tokens after a 48-token prompt,
median of 3 alternating runs with min-max.  That model is launch-bound: its weights are a few hundred KB.
usage: python profiles/qgemv_group_a8_rate.py [N=15] [--out FILE]   (GPU box; needs only the built tree).  Writes FILE (default
profiles/qgemv_group_a8_rate.txt) and prints the same lines."""
import json
import os
import statistics
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
out_arg = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
import qgemv_rate as base  # noqa: E402  (reads N from sys.argv; its --out default is not used here)
import torch  # noqa: E402
from gptq_gguf_toolkit_amd import ops  # noqa: E402

OUT = out_arg or os.path.join(HERE, "qgemv_group_a8_rate.txt")
H, KV, I = 4096, 1024, 14336
SHAPES = {"q": (H, H), "k": (KV, H), "v": (KV, H), "o": (H, H), "gate": (I, H), "up": (I, H), "down": (H, I)}
Q4, Q6 = 12, 14
CONFIGS = {"Q4_K": dict.fromkeys(SHAPES, Q4), "Q6_K": dict.fromkeys(SHAPES, Q6),
           "mix": dict(q=Q4, k=Q4, v=Q6, o=Q6, gate=Q4, up=Q4, down=Q6)}


def layer_ring(types, g):
    """[{name: blocks}]: distinct copies of one layer's packed weights."""
    first = {n: ops.pack(types[n], *ops.rtn_quantize(torch.randn(*SHAPES[n], device="cuda", generator=g) * 0.02, types[n])) for n in SHAPES}
    qkv = sum(first[n].numel() for n in "qkv")
    copies = max(-(-base.RING_BYTES // qkv) + 1, 2 * base.M)
    return [first] + [{n: b.clone() for n, b in first.items()} for _ in range(copies - 1)]


def parts(types, ring, x, xi):
    """{part: (group fn(i), single fn(i))}; x [T, H], xi [T, I]: the inputs of the launches."""
    W = lambda i: ring[i % len(ring)]  # noqa: E731
    one = lambda w, n, v: ops.gemv_packed_q8(types[n], w[n], v)  # noqa: E731
    qkv_g = lambda i: ops.gemv_packed_group_q8([(types[n], W(i)[n], None) for n in "qkv"], x)  # noqa: E731
    qkv_s = lambda i: [one(W(i), n, x) for n in "qkv"]  # noqa: E731
    sw_g = lambda i: ops.gemv_swiglu_packed_q8(types["gate"], W(i)["gate"], W(i)["up"], x)  # noqa: E731
    sw_s = lambda i: ops.fwd_silu_mul(one(W(i), "gate", x), one(W(i), "up", x))  # noqa: E731
    rest = lambda i: (one(W(i), "o", x), one(W(i), "down", xi))  # noqa: E731
    return {"qkv": (qkv_g, qkv_s), "swiglu": (sw_g, sw_s),
            "layer": (lambda i: (qkv_g(i), sw_g(i), rest(i)), lambda i: (qkv_s(i), sw_s(i), rest(i)))}


def flat(y):
    """The bits of every tensor of a (nested) result, in order."""
    return torch.cat([flat(t) for t in y]) if isinstance(y, (list, tuple)) else y.reshape(-1).view(torch.int16)


def tiny_llama_tokens_per_s(runs=3, new=64):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests", "golden"))
    from pathlib import Path
    from make_golden_shim import MIXED, tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd import generate, gguf_loader
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import convert
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    from gptq_gguf_toolkit_amd.quantizer import Quantizer
    from transformers import AutoModelForCausalLM
    load = lambda p: AutoModelForCausalLM.from_pretrained(p, dtype=torch.float16, attn_implementation="eager").cuda().eval()  # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        hf, sd = os.path.join(tmp, "hf"), os.path.join(tmp, "q")
        tiny_llama(dtype=torch.float16).save_pretrained(hf, safe_serialization=True)
        data = [([], {"input_ids": ids}) for ids in tiny_calib()]
        Quantizer(load(hf), data_loader=data, quantizable_modules=r".*layers.*((q|k|v|o|gate|up|down)_proj)$",
                  quantizer_kwargs=dict(rel_damp=0.01, block_size=128, act_order=False, quant_scale="absmax", static_groups=False,
                                        rmin=-1.0, rdelta=0.1, nstep=20, verbose=False),
                  pre_block_modules=["model.embed_tokens"], block_modules="model.layers", post_block_modules=["lm_head"],
                  quant_non_block_modules=True, device="cuda:0", save_dir=sd).quantize({k: T[v] for k, v in MIXED.items()})
        gguf = str(convert(Path(hf), Path(sd), Path(tmp) / "m.gguf", "f16", vocab=False))
        models = {k: gguf_loader.load_into_model(load(hf), gguf, packed=True, packed_decode_act="q8", packed_decode_group=k == "on")
                  for k in ("off", "on")}
    prompt = tiny_calib(n=1, L=48, seed=29)[0].cuda()
    ids = {k: generate.greedy(m, prompt, new) for k, m in models.items()}  # (and the warm-up)
    rates = {k: [] for k in models}
    for _ in range(runs):
        for k, m in models.items():
            t = {}
            generate.greedy(m, prompt, new, timings=t)
            rates[k].append((new - 1) / t["decode_s"])  # the one-token steps: wall time up to a device synchronise
    row = {"part": "tiny_llama_generate", "new_tokens": new, "runs": runs, "same_ids": bool(torch.equal(ids["off"], ids["on"]))}
    for k, r in rates.items():
        row[k] = {"tokens_per_s": round(statistics.median(r), 1), "min": round(min(r), 1), "max": round(max(r), 1)}
    row["on_over_off"] = round(row["on"]["tokens_per_s"] / row["off"]["tokens_per_s"], 3)
    return row


def main():
    lines = []
    g = torch.Generator(device="cuda").manual_seed(0)
    big = torch.randn(16384, 8192, device="cuda", generator=g).to(base.DT)
    blocker = lambda: torch.mm(big, big[:8192])  # noqa: E731
    for name, types in CONFIGS.items():
        ring = layer_ring(types, g)
        for T in (1, 4):
            x, xi = (torch.randn(T, c, device="cuda", generator=g).to(base.DT) for c in (H, I))
            plan = ops.gemv_group_a8_plan([types[n] for n in "qkv"], [SHAPES[n][0] for n in "qkv"], H, T)
            for part, (grp, single) in parts(types, ring, x, xi).items():
                if name == "mix" and part == "swiglu":
                    continue
                m = base.measure({"group": grp, "single": single}, blocker)
                row = {"types": name, "T": T, "part": part, "dtype": "bf16", "calls": base.N * base.M, "copies": len(ring),
                       "group": base.us(m["group"]), "single": base.us(m["single"]),
                       "group_over_single": round(m["group"][0] / m["single"][0], 3),
                       "equal": bool(torch.equal(flat(grp(0)), flat(single(0))))}
                if part == "qkv":
                    row["first_wg"] = plan["first_wg"]
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
        del ring
    lines.append(json.dumps(tiny_llama_tokens_per_s()))
    print(lines[-1], flush=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
