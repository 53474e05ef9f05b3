#!/usr/bin/env python3
"""gq_pack_bands against what the parent does with the same device tensors -- per band, the q / k row permute of five tensors
where it applies, then gq_pack -- on the walks of a Llama-3-8B block at five levels.  HIP events, a warm-up, then five
repeats alternating the two in one process (DESIGN.md 5c's method).  usage: python profiles/levelpack_bench.py [out.txt]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gptq_gguf_toolkit_amd import ops  # noqa: E402
from gptq_gguf_toolkit_amd.gguf_loader import rotary_row_dst  # noqa: E402
from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import permute  # noqa: E402

TYPES = [10, 11, 12, 13, 14]
TS = {10: 84, 11: 110, 12: 144, 13: 176, 14: 210}
SIGNED = {11, 14}


def walk(linears, C):
    """Random stacked outputs of one banded walk: `linears` = [(rows, heads or None)], Linear-major then level."""
    bands, gathers, r = [], [], 0
    for rows, heads in linears:
        for t in TYPES:
            r += rows
            bands.append((r, t))
            gathers.append(heads)
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randint(0, 4, (r, C), dtype=torch.uint8, device="cuda", generator=g)
    d = torch.randn(r, C // 256, device="cuda", generator=g).half()
    dmin = torch.randn(r, C // 256, device="cuda", generator=g).half()
    s = torch.randint(0, 16, (r * C // 16,), dtype=torch.uint8, device="cuda", generator=g)
    m = torch.randint(0, 16, (r * C // 16,), dtype=torch.uint8, device="cuda", generator=g)
    return (q, d, s, dmin, m), bands, gathers


def time_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(name, linears, C, say):
    stacked, bands, gathers = walk(linears, C)
    q, d, s, dmin, m = stacked
    lay, _ = ops.band_layout(bands, C)
    plan, total = ops.pack_bands_plan(bands, C)
    outs = torch.empty(total, dtype=torch.uint8, device="cuda")
    outs = [outs[off:off + nb] for *_, nb, off in plan]
    srcs = [None if h is None else rotary_row_dst("blk.0.attn_q.weight", r1 - r0, h, h, "cuda")
            for (r0, r1, *_), h in zip(lay, gathers)]

    def new():
        ops.pack_bands(stacked, bands, outs, srcs)

    def old():
        for (r0, r1, t, g, off), h in zip(lay, gathers):
            n = (r1 - r0) * (C // g)
            five = [q[r0:r1], d[r0:r1], s[off:off + n].view(r1 - r0, -1), dmin[r0:r1], m[off:off + n].view(r1 - r0, -1)]
            if h is not None:
                five = [permute(x, h, h) for x in five]
            ops.pack(t, *(five[:3] if t in SIGNED else five))

    new(), old()
    torch.cuda.synchronize()
    tn, to = [], []
    for _ in range(5):
        tn.append(time_ms(new))
        to.append(time_ms(old))
    params = q.numel()
    # ... plus what rides along: s (and m, dmin for the types that have them) and d
    moved = params + total + sum((r1 - r0) * ((C // g) + C // 256 * 2) * (1 if t in SIGNED else 2) for r0, r1, t, g, _ in lay)
    must = params + total  # 1 B/param read + type_size / 256 B/param written
    best = min(tn)
    say(f"{name}: R={q.shape[0]} C={C} {len(bands)} bands, {sum(h is not None for h in gathers)} gathered")
    say(f"  gq_pack_bands, one launch : {' '.join(f'{x:.3f}' for x in tn)} ms  (min {best:.3f}, spread {max(tn) - min(tn):.3f})")
    say(f"  per band permute + gq_pack: {' '.join(f'{x:.3f}' for x in to)} ms  (min {min(to):.3f}, spread {max(to) - min(to):.3f})")
    say(f"  bytes it must move {must / 1e9:.3f} GB (with scales {moved / 1e9:.3f} GB): {must / best / 1e6:.0f} GB/s at the best repeat")


def main():
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x)

    say(f"device: {torch.cuda.get_device_name(0)}")
    measure("gate/up walk of an 8B block, five levels", [(14336, None), (14336, None)], 4096, say)
    measure("q/k/v walk of an 8B block, five levels", [(4096, 32), (1024, 8), (1024, None)], 4096, say)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
