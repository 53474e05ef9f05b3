#!/usr/bin/env python3
"""ops.quad_form_experts (two launches whatever E) against the per-expert ops.quad_form loop (2 E launches) of the same
build: device time (HIP events around the calls) and wall time through the binding (perf_counter around the calls and one
synchronize), 3 warm-ups, median of 15 with the range, clocks as found.  B present (the numerator's call).

    python profiles/quad_form_experts_rate.py > profiles/quad_form_experts_rate.txt"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gptq_gguf_toolkit_amd import ops  # noqa: E402

CASES = ((8, 14336, 4096), (8, 4096, 14336), (128, 768, 2048), (128, 2048, 768))
WARM, REPS = 3, 15


def timed(fn):
    dev, wall = [], []
    for i in range(WARM + REPS):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i >= WARM:
            dev.append(a.elapsed_time(b) * 1e3)
            wall.append((t1 - t0) * 1e6)
    return dev, wall


def fmt(v):
    return f"{statistics.median(v):10.1f} [{min(v):9.1f} .. {max(v):9.1f}]"


def main():
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; bf16 A and fp16 B; microseconds, median [min .. max] of {REPS}")
    for E, R, C in CASES:
        A = torch.empty(E, R, C, device="cuda", dtype=torch.bfloat16).normal_(0, 0.02)
        B = (A.float() * 1.01).half()
        H = torch.empty(E, C, C, device="cuda").normal_()
        ws = torch.empty(int(E * ((R + 127) // 128) * (C // 128) * 8), dtype=torch.uint8, device="cuda")
        grouped = lambda: ops.quad_form_experts(A, H, B, ws=ws)  # noqa: E731
        loop = lambda: [ops.quad_form(A[e], H[e], B[e], ws=ws) for e in range(E)]  # noqa: E731
        same = torch.equal(grouped().view(torch.int64), torch.stack(loop()).view(torch.int64))
        gd, gw = timed(grouped)
        ld, lw = timed(loop)
        print(f"E={E:4d} R={R:6d} C={C:6d}  same bits: {same}")
        print(f"    grouped  device {fmt(gd)}   wall {fmt(gw)}")
        print(f"    loop     device {fmt(ld)}   wall {fmt(lw)}")
        print(f"    loop / grouped: device {statistics.median(ld) / statistics.median(gd):.3f}   wall "
              f"{statistics.median(lw) / statistics.median(gw):.3f}")
        del A, B, H, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
