#!/usr/bin/env python3
"""G17: the reference's three metrics, by RUNNING THE REFERENCE (read-only at /root/reference) on the CPU in fp32.

Imports evopress/src/metrics.py and runs compute_perplexity, compute_kl_div and compute_sparse_kl_div (top-k 32) on
make_golden_shim.tiny_llama() with tiny_calib()-style ids: seed 0 is the target model, seed 123 stands in for its quantized
version.  Stores DATA only -- the ids, both models' logits, the target's top-k pairs and the three returned floats -- as
tests/golden/G17_eval.npz (three sequences of 64 tokens, vocab 512: 384 KiB of fp32 logits per model).  Nothing of the
reference is copied.  Runs only where the reference is; the tests read the fixture.

Usage:  python tests/golden/make_golden_eval.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/evopress"
sys.path.insert(0, HERE)
sys.path.insert(0, REF)

from make_golden_shim import tiny_calib, tiny_llama  # noqa: E402
import src.metrics as ref_metrics  # noqa: E402

TOPK = 32


def main():
    data = tiny_calib(n=3, L=64, seed=17)
    target, quant = tiny_llama(seed=0), tiny_llama(seed=123)
    with torch.no_grad():
        t_logits = [target(ids).logits for ids in data]
        q_logits = [quant(ids).logits for ids in data]
    topk = [tuple(l.topk(k=TOPK, dim=-1)) for l in t_logits]
    ppl = ref_metrics.compute_perplexity(quant, data)
    kl = ref_metrics.compute_kl_div(quant, data, t_logits)
    skl = ref_metrics.compute_sparse_kl_div(quant, data, topk)
    # the batched forms of the reference agree with these to fp32 rounding (recorded, not used as anchors)
    ppl_b3 = ref_metrics.compute_perplexity(quant, data, batch_size=3)
    out = os.path.join(HERE, "G17_eval.npz")
    np.savez_compressed(
        out, ids=torch.cat(data).numpy(), target_logits=torch.cat(t_logits).numpy(), quant_logits=torch.cat(q_logits).numpy(),
        topk_values=torch.cat([v for v, _ in topk]).numpy(), topk_indices=torch.cat([i for _, i in topk]).numpy(),
        ppl=np.float64(ppl), kl=np.float64(kl), sparse_kl=np.float64(skl), ppl_batch3=np.float64(ppl_b3),
        meta=np.array(f"torch {torch.__version__} CPU fp32; evopress/src/metrics.py; tiny_llama seeds 0 (target) / 123; "
                      f"tiny_calib(n=3, L=64, seed=17); topk {TOPK}"))
    print(f"ppl {ppl!r} (batch 3: {ppl_b3!r})  kl {kl!r}  sparse_kl {skl!r}  -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
