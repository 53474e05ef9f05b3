"""The calibration forward of fused (dense bf16) experts at Mixtral-8x7B's shapes (E = 8, K = 2, H = 4096, I = 14336), one JSON
line per measurement:
  combine  ops.fwd_moe_combine (gq_fwd_moe_combine, one launch) against torch's chain of E x (multiply by the routing weight,
           cast, index_add_) on the same expert-sorted [P, H] matrix, the per-expert indices made beforehand; T = 4096.
  forward  one expert-module forward through moe_calibration.CalibExperts "routed" against "loop" (transformers'
           MixtralExperts.forward operation for operation, its host synchronisations included); T = 4096 and T = 512.  The two
           results are compared bit for bit first.
HIP events around one call, 3 warm-up calls, median of 15 with min-max, the candidates alternating, clocks as found.
usage: python profiles/moe_calib_rate.py [--out FILE]   (GPU box; needs only the built tree).  Writes FILE (default
profiles/moe_calib_rate.txt) and prints the same lines; the last line states the decision: "routed" is installed at the
`exact` level only if it is not slower than "loop" at T = 4096."""
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402
from gptq_gguf_toolkit_amd import moe_calibration as mc  # noqa: E402
from gptq_gguf_toolkit_amd import ops  # noqa: E402

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "moe_calib_rate.txt")
DT = torch.bfloat16
E, K, H, I = 8, 2, 4096, 14336
WARM, N = 3, 15


def measure(cands):
    keys = list(cands)
    for k in keys:
        for _ in range(WARM):
            cands[k]()
    torch.cuda.synchronize()
    times = {k: [] for k in keys}
    for it in range(N):
        for k in keys[it % len(keys):] + keys[:it % len(keys)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cands[k]()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e-3)
    return {k: {"us": round(statistics.median(v) * 1e6, 1), "min_us": round(min(v) * 1e6, 1), "max_us": round(max(v) * 1e6, 1)}
            for k, v in times.items()}


def routing(T, g):
    w, idx = torch.topk(torch.rand(T, E, device="cuda", generator=g), K, -1)  # uniformly random distinct experts
    return idx, (w / w.sum(-1, keepdim=True)).float()


@torch.no_grad()
def main():
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts
    lines = []
    g = torch.Generator(device="cuda").manual_seed(0)

    # ---- the combine alone
    T = 4096
    idx, w = routing(T, g)
    pairs = idx.t().to(torch.int32).contiguous().view(-1)
    route = ops.moe_route(pairs, E)
    y = torch.randn(T * K, H, device="cuda", generator=g).to(DT)
    where = [torch.where((idx == e).T) for e in range(E)]
    start = route[0].tolist()

    def chain():
        final = torch.zeros(T, H, dtype=DT, device="cuda")
        for e in range(E):
            top_k_pos, token_idx = where[e]
            h = y[start[e]:start[e + 1]] * w[token_idx, top_k_pos, None]
            final.index_add_(0, token_idx, h.to(DT))
        return final

    def kernel():
        return ops.fwd_moe_combine(y, pairs, route, w, E)

    same = bool(torch.equal(chain(), kernel()))
    m = measure({"kernel": kernel, "torch_chain": chain})
    byts = (K + 1) * T * H * 2
    lines.append(json.dumps({"what": "combine", "T": T, "K": K, "E": E, "H": H, "dtype": "bf16", "w": "fp32", "bit_identical": same,
                             **m, "kernel_GBps": round(byts / m["kernel"]["us"] / 1e3, 1),
                             "kernel_over_chain": round(m["kernel"]["us"] / m["torch_chain"]["us"], 3)}))
    print(lines[-1], flush=True)
    del y

    # ---- one expert-module forward
    with torch.device("cuda"):
        orig = MixtralExperts(MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=K)).to(DT)
    orig.gate_up_proj.normal_(0, 0.02, generator=g)
    orig.down_proj.normal_(0, 0.02, generator=g)
    loop, routed = mc.CalibExperts(orig, "loop"), mc.CalibExperts(orig, "routed")
    verdict = {}
    for T in (4096, 512):
        x = torch.randn(T, H, device="cuda", generator=g).to(DT)
        idx, w = routing(T, g)
        same = bool(torch.equal(loop(x, idx, w), routed._forward_routed(x, idx, w)))
        mc._routed_verdict[(T, K, E, H, I, DT)] = True  # the measurement times the trusted path, not the first-input check
        m = measure({"routed": lambda: routed(x, idx, w), "loop": lambda: loop(x, idx, w)})
        verdict[T] = m["routed"]["us"] <= m["loop"]["us"]
        lines.append(json.dumps({"what": "forward", "T": T, "K": K, "E": E, "H": H, "I": I, "dtype": "bf16", "bit_identical": same,
                                 **m, "routed_over_loop": round(m["routed"]["us"] / m["loop"]["us"], 3)}))
        print(lines[-1], flush=True)
    lines.append(json.dumps({"routed_not_slower_than_loop_at_T4096": verdict[4096], "routed_levels": list(mc.ROUTED_LEVELS)}))
    print(lines[-1], flush=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
