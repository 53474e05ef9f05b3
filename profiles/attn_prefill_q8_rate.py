#!/usr/bin/env python3
"""Prefill attention on the Q8_0 KV cache against the parent path, one layer at Llama-3-8B's attention shape (Hq 32, Hkv 8,
D 128, bf16, B = 1): a chunk of T query tokens that ends at position S of a filled cache.

    ours   : ops.attn_prefill_q8_0 over the packed cache (one launch, no workspace)
    parent : packed_kv_cache's fallback for the same call -- dequantize_blocks of the K and V slabs, repeat_interleave(G),
             torch SDPA with the materialised [T, S] boolean mask

Each point is the median of 15 timed calls (device events around one call, after 5 warm-up calls) with min .. max as the
spread; the two paths alternate call by call.  "peak MiB" is torch.cuda.max_memory_allocated above what is resident before the
call (the packed cache, q, the output).  "MFMA share" is the flops the causal attention needs, 4 D Hq sum_t (pos0 + t + 1), over
the kernel's time, over 2500 TFLOP/s -- the dense fp16 / bf16 matrix peak.  The last lines record, on a random 2-layer model of
the same attention shape, how far the logits of the last prompt token move when the prompt is fed in pieces of 512 on
Q8KVCache(prefill="q8_0") instead of in one forward (a record, not a test).  Writes the table to the file given as the first
argument (default: stdout only).

    python profiles/attn_prefill_q8_rate.py [out.txt]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gptq_gguf_toolkit_amd  # noqa: E402,F401
from gptq_gguf_toolkit_amd import ops  # noqa: E402

HQ, HKV, D, DT = 32, 8, 128, torch.bfloat16
G = HQ // HKV
PEAK = 2500e12
N, WARM = 15, 5
DEV = "cuda"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def point(T, S, kc, vc, lines):
    g = torch.Generator(device=DEV).manual_seed(S + T)
    pos0, scale, rb = S - T, D ** -0.5, ops.kv_row_bytes(D)
    q = torch.randn(1, T, HQ, D, generator=g, device=DEV).to(DT).transpose(1, 2)
    out = torch.empty(1, T, HQ, D, dtype=DT, device=DEV)

    def ours():
        ops.attn_prefill_q8_0(q, kc, vc, pos0, scale, out=out)

    def parent():
        k, v = (ops.dequantize_blocks(8, c[:, :, :S].reshape(-1, rb), DT).view(1, HKV, S, D).repeat_interleave(G, 1) for c in (kc, vc))
        mask = torch.ones(T, S, dtype=torch.bool, device=DEV).tril(S - T)
        return torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=scale).transpose(1, 2).contiguous()

    ref = parent().float()
    ours()
    diff = float((out.float() - ref).abs().max())
    del ref
    mem = {"ours": peak_mib(ours), "parent": peak_mib(parent)}
    for _ in range(WARM):
        ours(), parent()
    t = {"ours": [], "parent": []}
    for _ in range(N):
        t["ours"].append(timed(ours)), t["parent"].append(timed(parent))
    med = {k: statistics.median(v) for k, v in t.items()}
    flops = 4.0 * D * HQ * sum(pos0 + i + 1 for i in range(T))
    plan = ops.attn_prefill_plan(T, G)
    lines.append(f"{T:5d} {S:6d} | {med['ours']:9.1f} ({min(t['ours']):.1f} .. {max(t['ours']):.1f}) | {med['parent']:9.1f} "
                 f"({min(t['parent']):.1f} .. {max(t['parent']):.1f}) | {med['parent'] / med['ours']:5.2f}x | {mem['ours']:7.1f} "
                 f"{mem['parent']:8.1f} | {flops / (med['ours'] * 1e-6) / PEAK * 100:5.2f} % | {plan['blocks'] * HKV:4d} | {diff:.2e}")
    print(lines[-1], flush=True)


@torch.no_grad()
def chunked_against_one_shot(lines, L=2048, chunk=512):
    from transformers import LlamaConfig, LlamaForCausalLM
    from gptq_gguf_toolkit_amd import packed_kv_cache as pk
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=HQ * D, intermediate_size=2048, num_hidden_layers=2, num_attention_heads=HQ, num_key_value_heads=HKV,
                      vocab_size=2048, max_position_embeddings=L, tie_word_embeddings=False)
    model = LlamaForCausalLM(cfg).to(DT).to(DEV).eval()
    ids = torch.randint(0, 2048, (1, L), generator=torch.Generator().manual_seed(1)).to(DEV)
    rows = {}
    for name, prefill, step in (("one forward", "sdpa", L), ("pieces, prefill='sdpa'", "sdpa", chunk), ("pieces, prefill='q8_0'", "q8_0", chunk)):
        cache = pk.install(model, pk.Q8KVCache(cfg, 1, L, device=DEV, prefill=prefill))
        try:
            for i in range(0, L, step):
                out = model(input_ids=ids[:, i:i + step], past_key_values=cache, use_cache=True, logits_to_keep=1)
        finally:
            pk.restore(model)
        rows[name] = out.logits[:, -1].float()
    one = rows.pop("one forward")
    for name, r in rows.items():
        lines.append(f"random 2-layer model, prompt {L} in pieces of {chunk}: max |logit - one forward's| {name}: "
                     f"{float((r - one).abs().max()):.3e} (max |logit| {float(one.abs().max()):.2f})")
        print(lines[-1], flush=True)


def main():
    assert torch.cuda.is_available(), "attn_prefill_q8_rate needs a GPU"
    lines = [f"one layer, Hq {HQ} Hkv {HKV} D {D} bf16, B = 1; times in us, median of {N} (min .. max); {torch.cuda.get_device_name(0)}",
             "    T      S | attn_prefill_q8_0 (ours)       | decode + repeat + SDPA with mask (parent) | parent / ours | peak MiB ours "
             "parent | MFMA share of 2500 TFLOP/s | workgroups | max |ours - parent|"]
    print("\n".join(lines), flush=True)
    for S in (4096, 32768):
        g = torch.Generator(device=DEV).manual_seed(S)
        kc, vc = (torch.zeros(1, HKV, S, ops.kv_row_bytes(D), dtype=torch.uint8, device=DEV) for _ in range(2))
        ops.kv_append_q8_0(kc, vc, *(torch.randn(1, HKV, S, D, generator=g, device=DEV).to(DT) for _ in range(2)), 0)
        for T in (512, 2048):
            point(T, S, kc, vc, lines)
        del kc, vc
    chunked_against_one_shot(lines)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
