"""Qwen3's per-head q / k RMSNorm + rotary embedding at Qwen3-8B's attention shape (Hq = 32, Hkv = 8, D = 128, bf16), one JSON
line per measurement:
  op      ops.fwd_qk_norm_rope (gq_fwd_qk_norm_rope, ONE launch for q and k) against what --fused_forward exact ran for the same
          work before that kernel: two eager Qwen3RMSNorm calls (head_dim 128 is not a width gq_fwd_rmsnorm_ordered takes) and
          two ops.fwd_rope launches; B x L = 1 x 2048, 1 x 8192 and 4 x 2048 (cos / sin of batch 1, expanded as the model
          patch expands them).  The two results are compared bit for bit first.  bytes = one read and one write of q and k plus
          one read of cos / sin per token; floor_us = bytes at 6.29 TB/s (the float4-copy rate of an MI355X).
  model   Quantizer.quantize of the tiny Qwen3 of tests/tiny_qwen3.py (2 layers, hidden 256, fp16), fused_forward "exact" with
          the kernel installed against the same level without it (forward_fused.QK_NORM_ROPE_IN_EXACT = False): wall seconds,
          median of 3, alternating.
HIP events around one call, 3 warm-up calls, median of 15 with min-max, the candidates alternating, clocks as found.
usage: python profiles/qk_norm_rope_rate.py [--out FILE]   (GPU box; needs only the built tree).  Writes FILE (default
profiles/qk_norm_rope_rate.txt) and prints the same lines; the last line states the decision: the kernel stays in the "exact"
level only if it is not slower than the parent path at all three points."""
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import torch  # noqa: E402
from gptq_gguf_toolkit_amd import forward_fused, ops  # noqa: E402

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "qk_norm_rope_rate.txt")
DT = torch.bfloat16
HQ, HK, D, EPS = 32, 8, 128, 1e-6
HBM = 6.29e12
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


def quantize_wall(kernel_on):
    import tiny_qwen3 as TQ
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    from gptq_gguf_toolkit_amd.quantizer import Quantizer
    forward_fused.QK_NORM_ROPE_IN_EXACT = kernel_on
    model = TQ.tiny_qwen3(dtype=torch.float16).cuda()
    data = [([], {"input_ids": ids}) for ids in TQ.tiny_calib()]
    with tempfile.TemporaryDirectory() as d:
        drv = Quantizer(model, data_loader=data, quantizable_modules=TQ.LINEARS,
                        quantizer_kwargs=dict(rel_damp=0.01, block_size=128, act_order=False, quant_scale="absmax",
                                              static_groups=False, rmin=-1.0, rdelta=0.1, nstep=20, verbose=False),
                        pre_block_modules=["model.embed_tokens"], block_modules="model.layers", post_block_modules=["lm_head"],
                        quant_non_block_modules=True, device="cuda:0", save_dir=d, fused_forward="exact")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        drv.quantize({k: T.Q4_K for k in ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj",
                                          "embed_tokens", "lm_head")})
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    assert ("Qwen3Attention.forward" in " ".join(drv._fused_modules)) == kernel_on
    return dt


@torch.no_grad()
def main():
    from transformers.models.qwen3 import modeling_qwen3 as M
    lines, not_slower = [], []
    g = torch.Generator(device="cuda").manual_seed(0)
    nq, nk = M.Qwen3RMSNorm(D, eps=EPS).to("cuda", DT), M.Qwen3RMSNorm(D, eps=EPS).to("cuda", DT)
    nq.weight.copy_(1.0 + 0.2 * torch.randn(D, device="cuda", generator=g))
    nk.weight.copy_(1.0 + 0.2 * torch.randn(D, device="cuda", generator=g))
    inv = 1.0 / (1000000.0 ** (torch.arange(0, D, 2, device="cuda").float() / D))
    for B, L in ((1, 2048), (1, 8192), (4, 2048)):
        q = torch.randn(B, L, HQ, D, device="cuda", generator=g).to(DT)
        k = torch.randn(B, L, HK, D, device="cuda", generator=g).to(DT)
        ang = torch.arange(L, device="cuda").float()[None, :, None] * inv[None, None, :]
        emb = torch.cat([ang, ang], -1)
        cos, sin = emb.cos().to(DT), emb.sin().to(DT)  # [1, L, D]

        def fused():
            c, s = cos.expand(B, L, D).contiguous(), sin.expand(B, L, D).contiguous()
            return ops.fwd_qk_norm_rope(q, k, nq.weight, nk.weight, c, s, EPS)

        def parent():  # forward_fused._rope's own steps after the two eager norms
            c, s = cos.expand(B, L, D).contiguous(), sin.expand(B, L, D).contiguous()
            return ops.fwd_rope(nq(q), c, s), ops.fwd_rope(nk(k), c, s)

        a, b = fused(), parent()
        same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
        t = measure({"kernel": fused, "parent": parent})
        nbytes = 2 * 2 * B * L * (HQ + HK) * D + 2 * 2 * B * L * D
        rec = {"what": "op", "B": B, "L": L, "Hq": HQ, "Hkv": HK, "D": D, "dtype": "bf16", "bit_identical": same, "kernel": t["kernel"],
               "parent_2_eager_norms_2_fwd_rope": t["parent"], "bytes": nbytes, "floor_us": round(nbytes / HBM * 1e6, 1),
               "kernel_GBps": round(nbytes / (t["kernel"]["us"] * 1e-6) / 1e9, 1),
               "kernel_over_parent": round(t["kernel"]["us"] / t["parent"]["us"], 3)}
        not_slower.append(same and t["kernel"]["us"] <= t["parent"]["us"])
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    walls = {True: [], False: []}
    quantize_wall(True)  # warm-up: code objects, allocator
    for _ in range(3):
        for on in (True, False):
            walls[on].append(quantize_wall(on))
    forward_fused.QK_NORM_ROPE_IN_EXACT = True
    lines.append(json.dumps({"what": "model", "model": "tiny Qwen3 (2 layers, hidden 256, fp16), 8 x 64 calibration tokens",
                             "kernel_on_s": {"median": round(statistics.median(walls[True]), 3), "all": [round(x, 3) for x in walls[True]]},
                             "kernel_off_s": {"median": round(statistics.median(walls[False]), 3), "all": [round(x, 3) for x in walls[False]]}}))
    print(lines[-1], flush=True)
    lines.append(json.dumps({"kernel_not_slower_than_parent_at_all_three_points": all(not_slower),
                             "qk_norm_rope_levels": ["exact", "all"] if all(not_slower) else ["all"]}))
    print(lines[-1], flush=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
