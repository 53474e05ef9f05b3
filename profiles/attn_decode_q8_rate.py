#!/usr/bin/env python3
"""Decode attention on the Q8_0 KV cache against the parent path, one layer at Llama-3-8B's attention shape (Hq 32, Hkv 8,
D 128, bf16), T = 1:

    ours   : ops.kv_append_q8_0 of the new row + ops.attn_decode_q8_0 over the packed cache
    parent : DynamicLayer.update (torch.cat of the 16-bit cache with the new row) + torch SDPA (enable_gqa) on the result

Each point is the median of 15 timed calls (device events around one call, after 5 warm-up calls) with min .. max as the
spread; the two paths alternate call by call.  "HBM fraction" is the packed bytes of K and V the kernel must read, over the
attention kernels' time (the decode call alone, timed the same way), over 8.0 TB/s -- a share of the peak stream rate, not
of a measured copy rate.  Writes the table to the file given as the first argument (default: stdout only).

    python profiles/attn_decode_q8_rate.py [out.txt]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gptq_gguf_toolkit_amd  # noqa: E402,F401
from gptq_gguf_toolkit_amd import ops  # noqa: E402

HQ, HKV, D, DT = 32, 8, 128, torch.bfloat16
HBM = 8.0e12
N, WARM = 15, 5


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def point(B, S, lines):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(S + B)
    pos0 = S - 1
    kb, vb = (torch.randn(B, HKV, pos0, D, generator=g, device=dev).to(DT) for _ in range(2))
    kn, vn = (torch.randn(B, 1, HKV, D, generator=g, device=dev).to(DT).transpose(1, 2) for _ in range(2))
    q = torch.randn(B, 1, HQ, D, generator=g, device=dev).to(DT).transpose(1, 2)
    kc, vc = (torch.zeros(B, HKV, (S + 3) // 4 * 4, ops.kv_row_bytes(D), dtype=torch.uint8, device=dev) for _ in range(2))
    ops.kv_append_q8_0(kc, vc, kb, vb, 0)
    ws = torch.empty(ops.attn_decode_workspace_bytes(S, B, HKV, HQ // HKV, D), dtype=torch.uint8, device=dev)
    out = torch.empty(B, 1, HQ, D, dtype=DT, device=dev)
    scale = D ** -0.5

    def ours():
        ops.kv_append_q8_0(kc, vc, kn, vn, pos0)
        ops.attn_decode_q8_0(q, kc, vc, pos0, scale, out=out, ws=ws)

    def attn_only():
        ops.attn_decode_q8_0(q, kc, vc, pos0, scale, out=out, ws=ws)

    def parent():
        k, v = torch.cat([kb, kn], -2), torch.cat([vb, vn], -2)
        return torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=scale, enable_gqa=True)

    ref = parent().transpose(1, 2).float()
    ours()
    diff = float((out.float() - ref).abs().max())
    for _ in range(WARM):
        ours(), attn_only(), parent()
    t = {"ours": [], "attn": [], "parent": []}
    for _ in range(N):
        t["ours"].append(timed(ours)), t["parent"].append(timed(parent)), t["attn"].append(timed(attn_only))
    med = {k: statistics.median(v) for k, v in t.items()}
    packed, dense = 2 * B * HKV * S * ops.kv_row_bytes(D), 2 * B * HKV * S * D * 2
    plan = ops.attn_decode_plan(S, B, HKV, HQ // HKV)
    lines.append(f"{S:6d} {B:2d} | {med['ours']:9.1f} ({min(t['ours']):.1f} .. {max(t['ours']):.1f}) | {med['parent']:9.1f} "
                 f"({min(t['parent']):.1f} .. {max(t['parent']):.1f}) | {med['parent'] / med['ours']:5.2f}x | {med['attn']:9.1f} "
                 f"({min(t['attn']):.1f} .. {max(t['attn']):.1f}) {packed / (med['attn'] * 1e-6) / HBM * 100:5.1f} % | "
                 f"{packed / 2**20:8.1f} {dense / 2**20:8.1f} | {plan['splits']:2d} x {plan['chunk']:5d} | {diff:.2e}")
    print(lines[-1], flush=True)


def main():
    assert torch.cuda.is_available(), "attn_decode_q8_rate needs a GPU"
    lines = [f"one layer, Hq {HQ} Hkv {HKV} D {D} bf16, T = 1; times in us, median of {N} (min .. max); {torch.cuda.get_device_name(0)}",
             "context B | append + decode (ours)   | cat + SDPA, 16-bit cache (parent) | parent / ours | decode alone, share of 8.0 TB/s on "
             "the packed bytes | cache MiB packed / 16-bit | plan splits x chunk | max |ours - parent|"]
    print("\n".join(lines), flush=True)
    for S in (512, 4096, 32768):
        for B in (1, 8):
            point(B, S, lines)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
