"""K16 scoring rates on the GPU, one JSON line.  Shapes: [2047, 128256] (one 2048-token Llama-3 sequence) in fp16 and bf16,
and [8 * 2047, 32000] in fp16.  In one process, HIP events around each call, warm-up first, the candidates ALTERNATING,
median of N calls each:
  nll        gq_eval_nll                          vs  F.cross_entropy(logits, labels, reduction="none")
  kl         gq_eval_kl                           vs  the reference's dense KL block, 1024-row chunks included
                                                      (evopress/src/metrics.py:66-83 without its empty_cache calls)
  kl_sparse  gq_eval_kl_sparse (top-k 32 / 4096)  vs  logits.gather(-1, ids) + the same KL expression
Rates are algorithmic bytes (every operand read once) over the median time, as a fraction of the 6.3 TB/s streaming
figure of the chip; 0.5 GB operands do not fit the 256 MiB Infinity Cache.  gq_eval_nll's time includes the stream wait
it ends with.
usage: python profiles/eval_rate.py [N=15]   (GPU box; needs only the built tree)"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from gptq_gguf_toolkit_amd import ops  # noqa: E402

STREAM = 6.3e12
N = int(sys.argv[1]) if len(sys.argv) > 1 else 15


def ref_kl_chunked(x, t):
    """The reference's block: log_softmax of both, F.kl_div, 1024 rows at a time."""
    out = []
    for i in range(0, x.shape[0], 1024):
        xb, tb = x[i:i + 1024], t[i:i + 1024]
        out.append(F.kl_div(xb.log_softmax(dim=-1), tb.log_softmax(dim=-1), log_target=True, reduction="batchmean"))
    return torch.stack(out)


def ref_kl_sparse(x, vals, ids):
    g = x.gather(dim=-1, index=ids)
    return F.kl_div(g.log_softmax(dim=-1), vals.log_softmax(dim=-1), log_target=True, reduction="batchmean")


def main():
    res = {"calls": N, "streaming_TBps": STREAM / 1e12, "shapes": []}
    for T, V, dt, K in ((2047, 128256, torch.float16, 32), (2047, 128256, torch.bfloat16, 4096), (8 * 2047, 32000, torch.float16, 32)):
        torch.manual_seed(0)
        t = (torch.randn(T, V, device="cuda") * 3).to(dt)
        x = (t.float() + 0.1 * torch.randn(T, V, device="cuda")).to(dt)
        labels = torch.randint(0, V, (T,), device="cuda")
        vals, ids = t.topk(k=K, dim=-1)
        es = x.element_size()
        cands = {
            "nll": (lambda: ops.eval_nll(x, labels), T * V * es),
            "torch_nll": (lambda: F.cross_entropy(x, labels, reduction="none"), None),
            "kl": (lambda: ops.eval_kl(x, t), 2 * T * V * es),
            "torch_kl": (lambda: ref_kl_chunked(x, t), None),
            "kl_sparse": (lambda: ops.eval_kl_sparse(x, vals, ids), T * K * (2 * es + 8)),
            "torch_kl_sparse": (lambda: ref_kl_sparse(x, vals, ids), None),
        }
        for fn, _ in cands.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times, keys = {k: [] for k in cands}, list(cands)
        for it in range(N):
            evs = []
            for k in keys[it % len(keys):] + keys[:it % len(keys)]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                cands[k][0]()
                e1.record()
                evs.append((k, e0, e1))
            torch.cuda.synchronize()
            for k, e0, e1 in evs:
                times[k].append(e0.elapsed_time(e1) * 1e-3)
        row = {"T": T, "V": V, "dtype": str(dt).replace("torch.", ""), "K": K}
        for k in ("nll", "kl", "kl_sparse"):
            med, tmed = statistics.median(times[k]), statistics.median(times["torch_" + k])
            nbytes = cands[k][1]
            row[k] = {"ms": round(med * 1e3, 4), "torch_ms": round(tmed * 1e3, 4), "torch_over_ours": round(tmed / med, 2),
                      "TBps": round(nbytes / med / 1e12, 3), "of_streaming": round(nbytes / med / STREAM, 3)}
        res["shapes"].append(row)
        del t, x, vals, ids
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
