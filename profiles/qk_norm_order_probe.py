"""Which summation order does ATen's mean(-1) use for a contiguous fp32 [rows, D] tensor at the head sizes of a per-head
RMSNorm (D = 64 / 128 / 256), and does it depend on the number of rows?  Candidate orders are emulated with torch ops
(explicit fp32 adds in a fixed order) and compared bitwise with torch's own sum and mean; then gq_fwd_qk_norm_rope's
statistics and outputs are compared with the eager expressions at the same sizes.  (GPU box)"""
import itertools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gptq_gguf_toolkit_amd import ops  # noqa: E402

g = torch.Generator(device="cuda").manual_seed(0)


def cand(p, B, vec, tree, fold):
    """B lanes per row; lane x adds elements (x + B it) vec + j into accumulator j; the accumulators folded `fold`; the lanes
    folded with shuffle-down offsets in `tree` order."""
    rows, C = p.shape
    if C % (B * vec):
        return None
    it = C // (B * vec)
    v = p.view(rows, it, B, vec)
    acc = v[:, 0].clone()
    for i in range(1, it):
        acc = acc + v[:, i]
    if fold == "seq":
        s = acc[..., 0]
        for j in range(1, vec):
            s = s + acc[..., j]
    else:
        a = acc
        while a.shape[-1] > 1:
            a = a[..., 0::2] + a[..., 1::2]
        s = a[..., 0]
    offs = [1 << k for k in range(B.bit_length() - 1)]
    if tree == "dec":
        offs = offs[::-1]
    for o in offs:
        s = s + torch.cat([s[:, o:], s[:, -o:]], dim=1)  # lane i reads lane i + o (the tail does not reach lane 0)
    return s[:, 0]


print("== order of mean(-1), fp32 [rows, D]")
for D in (64, 128, 256):
    for rows in (1, 2, 3, 7, 8, 15, 16, 33, 264, 1056, 16384, 81920):
        x = torch.randn(rows, D, device="cuda", generator=g)
        p = x.pow(2)
        want_sum, want_mean = p.sum(-1), p.mean(-1)
        hits = []
        for B, vec, tree, fold in itertools.product((8, 16, 32, 64, 128, 256), (1, 2, 4, 8), ("inc", "dec"), ("seq", "pair")):
            if B == 1 or (vec == 1 and fold == "pair") or (B <= 2 and tree == "dec"):
                continue
            s = cand(p, B, vec, tree, fold)
            if s is not None and torch.equal(s, want_sum):
                hits.append((B, vec, tree, fold))
        fac = torch.tensor(1.0 / D, device="cuda")
        print(f"D={D} rows={rows}: hits {hits[:5]} | mean == sum * (1/D): {torch.equal(want_sum * fac, want_mean)}", flush=True)

print("== gq_fwd_qk_norm_rope against the eager expressions")
from transformers.models.qwen3 import modeling_qwen3 as mq  # noqa: E402

for D, dt, (B, L, Hq, Hk) in itertools.product((64, 128, 256), (torch.bfloat16, torch.float16),
                                               ((1, 1, 1, 1), (1, 8, 4, 2), (2, 33, 8, 2), (1, 2048, 32, 8))):
    q = torch.randn(B, L, Hq, D, device="cuda", generator=g).to(dt)
    k = torch.randn(B, L, Hk, D, device="cuda", generator=g).to(dt)
    nq, nk = mq.Qwen3RMSNorm(D).to("cuda", dt), mq.Qwen3RMSNorm(D).to("cuda", dt)
    with torch.no_grad():
        nq.weight.copy_(torch.randn(D, device="cuda", generator=g))
        nk.weight.copy_(torch.randn(D, device="cuda", generator=g))
        ang = torch.randn(B, L, D, device="cuda", generator=g)
        cos, sin = ang.cos().to(dt), ang.sin().to(dt)
        want = mq.apply_rotary_pos_emb(nq(q).transpose(1, 2), nk(k).transpose(1, 2), cos, sin)
        gq_, gk_, stats = ops.fwd_qk_norm_rope(q, k, nq.weight, nk.weight, cos, sin, nq.variance_epsilon, want_stats=True)
        var = torch.cat([q.float().pow(2).mean(-1).reshape(-1), k.float().pow(2).mean(-1).reshape(-1)])
        r = torch.rsqrt(var + nq.variance_epsilon)
    print(f"D={D} {dt} B={B} L={L} Hq={Hq} Hk={Hk}: q {torch.equal(want[0].transpose(1, 2), gq_)} k {torch.equal(want[1].transpose(1, 2), gk_)} "
          f"var {torch.equal(stats[:, 0], var)} ({int((stats[:, 0] != var).sum())} of {var.numel()} rows differ) "
          f"r {torch.equal(stats[:, 1], r)}", flush=True)
