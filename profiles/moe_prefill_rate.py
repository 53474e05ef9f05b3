"""One whole expert FFN of a packed MoE layer's PREFILL (gate, up, activation, down, weighted sum over k) three ways: one JSON
line per (type, T).
  grouped  PackedExperts.forward with prefill = "grouped"      -- K25: gq_moe_route + three gq_linear_packed_experts launches per chunk
  loop     the same PackedExperts with prefill = "loop"        -- the per-expert loop over ops.linear_packed / gemv_packed on slice
                                                                  views, its host synchronisations (unique, where) included
  hf       transformers' MixtralExperts.forward (its own loop) -- on the decoded bf16 weights, host synchronisations included
at Mixtral-8x7B's shapes: E = 8, K = 2, gate / up [14336, 4096], down [4096, 14336]; Q4_K and Q6_K, bf16, T in {64, 512, 2048,
8192}, uniformly random distinct experts per token (one routing per T, seeded).
Method of profiles/moe_gemv_rate.py: one process, HIP events, warm-up first, the candidates alternating, median of N with min-max,
clocks as found; a measurement is M back-to-back calls between two events, divided by M, each batch enqueued behind a matrix
product of a few milliseconds so that the events of the candidate without host synchronisation bracket device time alone (a
candidate that synchronises drains that product first and is then timed as a forward would run it: device time plus the host's
round trips).  Cold weights: a prefill reads every expert, 0.79 GB (Q4_K) or 1.15 GB (Q6_K) of packed bytes per layer and call,
and every candidate rotates through COPIES = 2 layers: well over 512 MiB of other bytes pass between two uses of the same bytes
(the last-level cache is 256 MiB).  TFLOP/s is algorithmic: 2 * T * K * 3 * I * H over the median time.
usage: python profiles/moe_prefill_rate.py [N=7] [--out FILE] [--only grouped] [--tag NAME]   (GPU box; needs only the built tree;
--only grouped with GQ_SO_PATH set to a probe build of profiles/micro/build_moe_gemm_probes.sh times one token-tile width).
Writes FILE (default profiles/moe_prefill_rate.txt) and prints the same lines; the last line names the points where the grouped
path lost to the loop."""
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402
from gptq_gguf_toolkit_amd import ops  # noqa: E402
from gptq_gguf_toolkit_amd.packed_experts import ROLES, PackedExperts  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdecimal() else 7
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "moe_prefill_rate.txt")
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
TAG = sys.argv[sys.argv.index("--tag") + 1] if "--tag" in sys.argv else None
DT = torch.bfloat16
NAMES = {12: "Q4_K", 14: "Q6_K"}
E, K, H, I = 8, 2, 4096, 14336
COPIES, M = 2, 2
TS = (64, 512, 2048, 8192)


def hf_experts():
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts
    with torch.device("meta"):
        mod = MixtralExperts(MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=K))
    del mod._parameters["gate_up_proj"], mod._parameters["down_proj"]  # plain attributes: a copy's tensors are put there per call
    loop = getattr(MixtralExperts.forward, "__wrapped__", MixtralExperts.forward)  # the class's own loop, whatever the config dispatches to
    return mod, loop


def measure(cands, blocker):
    """cands: {name: fn(i)}, i the call's number (it picks the copy of the layer)."""
    keys, calls = list(cands), 0
    for k in keys:
        for _ in range(2):
            cands[k](calls)
            calls += 1
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for it in range(N):
        evs = []
        for k in keys[it % len(keys):] + keys[:it % len(keys)]:
            blocker()
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


@torch.no_grad()
def main():
    lines, lost = [], []
    g = torch.Generator(device="cuda").manual_seed(0)
    big = torch.randn(16384, 8192, device="cuda", generator=g).to(DT)
    blocker = lambda: torch.mm(big, big[:8192])  # noqa: E731
    hf, hf_loop = hf_experts()
    for t in NAMES:
        layers, dense = [], []
        for c in range(COPIES):
            mod = PackedExperts(E, H, I, DT)
            for role in ROLES:
                R, C = mod.role_shape(role)
                W = torch.randn(E * R, C, device="cuda", generator=g) * 0.02
                mod.set_level(role, ops.pack(t, *ops.rtn_quantize(W, t)).view(-1), t)
                del W
            layers.append(mod)
            if ONLY is None:
                dense.append((mod.dense_gate_up(), mod.dense_weight("down")))
        for T in TS:
            x = torch.randn(T, H, device="cuda", generator=g).to(DT)
            w, idx = torch.topk(torch.rand(T, E, device="cuda", generator=g), K, -1)  # uniformly random distinct experts
            w = w / w.sum(-1, keepdim=True)
            counts = torch.bincount(idx.reshape(-1), minlength=E).tolist()

            def grouped(i):
                mod = layers[i % COPIES]
                mod.prefill = "grouped"
                try:
                    return mod(x, idx, w)
                finally:
                    del mod.prefill

            def loop(i):
                return layers[i % COPIES](x, idx, w)

            def hf_call(i):
                hf.gate_up_proj, hf.down_proj = dense[i % COPIES]
                return hf_loop(hf, x, idx, w)

            assert PackedExperts.prefill == "loop" and not layers[0].takes_decode_path(T, K)
            cands = {"grouped": grouped, "loop": loop, "hf": hf_call}
            if ONLY is not None:
                cands = {ONLY: cands[ONLY]}
            m = measure(cands, blocker)
            flop = 2.0 * T * K * 3 * I * H
            row = {"type": NAMES[t], "E": E, "K": K, "H": H, "I": I, "T": T, "dtype": "bf16", "pairs_per_expert": counts,
                   "chunks": -(-T * K // PackedExperts.prefill_max_pairs), "calls": N * M, "copies": COPIES}
            if TAG:
                row["tag"] = TAG
            for k in m:
                row[k] = us(m[k])
                row[k + "_TFLOPs"] = round(flop / m[k][0] / 1e12, 1)
            if ONLY is None:
                row["grouped_over_loop"] = round(m["grouped"][0] / m["loop"][0], 3)
                row["grouped_over_hf"] = round(m["grouped"][0] / m["hf"][0], 3)
                if m["grouped"][0] > m["loop"][0]:
                    lost.append((NAMES[t], T))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
        hf.gate_up_proj = hf.down_proj = None
        del layers, dense
        torch.cuda.empty_cache()
    if ONLY is None:
        lines.append(json.dumps({"grouped_no_slower_than_loop_at_every_point": not lost, "points_lost": lost,
                                 "prefill_default": PackedExperts.prefill, "prefill_max_pairs": PackedExperts.prefill_max_pairs}))
        print(lines[-1], flush=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
