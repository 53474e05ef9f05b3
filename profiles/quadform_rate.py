"""K17 quadratic-form rates on the GPU, one JSON line.  Shapes (R x C): 4096 x 14336, 14336 x 4096, 4096 x 4096 (the Linears
of a Llama-3-8B block), A and B fp16, H fp32 [C, C].  In one process, HIP events around each call, warm-up first, the two
candidates ALTERNATING, median of N calls each:
  quad_form  gq_quad_form(A, B, H)   vs   D = A.float() - B.float(); ((D @ H) * D).sum()   (the reference's line, TF32 off)
Rates are algorithmic flops R C^2 (the symmetric half; the torch form does 2 R C^2) over the median time, as a fraction of
the 157.3 TFLOP/s fp32 MFMA peak.  torch_peak_MiB is what the torch form allocates on top of its operands.
usage: python profiles/quadform_rate.py [N=15]   (GPU box; needs only the built tree)"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from gptq_gguf_toolkit_amd import ops  # noqa: E402

PEAK = 157.3e12
N = int(sys.argv[1]) if len(sys.argv) > 1 else 15


def torch_form(A, B, H):
    D = A.float() - B.float()
    return ((D @ H) * D).sum()


def main():
    assert torch.backends.cuda.matmul.allow_tf32 is False
    res = {"calls": N, "peak_TFLOPs": PEAK / 1e12, "shapes": []}
    for R, C in ((4096, 14336), (14336, 4096), (4096, 4096)):
        torch.manual_seed(0)
        X = torch.randn(2 * C, C, device="cuda", dtype=torch.float16)
        H = ops.h_accumulate(torch.zeros(C, C, device="cuda"), X, 0.0, 1.0 / C)
        del X
        A = (torch.randn(R, C, device="cuda") * 0.02).half()
        B = (A.float() + 2e-4 * torch.randn(R, C, device="cuda")).half()
        cands = {"quad_form": lambda: ops.quad_form(A, H, B), "torch": lambda: torch_form(A, B, H)}
        for fn in cands.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        v_t = torch_form(A, B, H).item()
        peak = torch.cuda.max_memory_allocated() - base
        v_k = ops.quad_form(A, H, B).item()
        times = {k: [] for k in cands}
        for _ in range(N):
            for k, fn in cands.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
        med = {k: statistics.median(v) for k, v in times.items()}
        res["shapes"].append({
            "R": R, "C": C, "quad_form_ms": round(med["quad_form"], 4), "torch_ms": round(med["torch"], 4),
            "quad_form_min_ms": round(min(times["quad_form"]), 4), "torch_min_ms": round(min(times["torch"]), 4),
            "quad_form_TFLOPs": round(R * C * C / med["quad_form"] / 1e9, 2),
            "quad_form_of_peak": round(R * C * C / (med["quad_form"] * 1e-3) / PEAK, 4),
            "torch_peak_MiB": round(peak / 2 ** 20, 1), "speedup": round(med["torch"] / med["quad_form"], 3),
            "rel_diff_values": abs(v_k - v_t) / abs(v_k)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
