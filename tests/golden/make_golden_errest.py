#!/usr/bin/env python3
"""G18: the reference's layer error estimate, by RUNNING THE REFERENCE (read-only at /root/reference) on the CPU in fp32.

Imports evopress/src/error_estimator.py and runs its LayerErrorEstimator on one nn.Linear(256, 48): two update() calls
with [1, 320, 256] inputs whose column 37 is all zero (a dead channel; 640 tokens > 256 columns, so H is positive
definite apart from it and every row's term is >= 0), pre_step(), and estimate() for three W_c = W + sigma * noise,
sigma = 1e-1, 1e-2, 1e-3 of W's RMS.  Stores DATA only -- the inputs (fp16-representable values, kept as fp16), W, the three W_c, H after pre_step, the three
returned floats, and in `rel_dist` the relative distance of each float from the same expression in fp64 on the stored
inputs (the reference's own fp32 error: the bound of the tests comes from it) -- as tests/golden/G18_errest.npz.
Nothing of the reference is copied.  Runs only where the reference is; the tests read the fixture.

Usage:  python tests/golden/make_golden_errest.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/evopress"
sys.path.insert(0, REF)

from src.error_estimator import LayerErrorEstimator  # noqa: E402

DEAD = 37
SIGMAS = (1e-1, 1e-2, 1e-3)


def fp64_estimate(xs, W, W_c):
    """error_estimator.py:65-69, 88-89, 101-103 in fp64 on fp32 data."""
    H, n = torch.zeros(W.shape[1], W.shape[1], dtype=torch.float64), 0
    for x in xs:
        x2 = x.reshape(-1, x.shape[-1]).double()
        b = x.shape[0]
        H = H * (n / (n + b)) + (2.0 / (n + b)) * (x2.T @ x2)
        n += b
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    D, Wd = (W - W_c).double(), W.double()  # the reference subtracts in fp32
    return float(((D @ H) * D).sum() / ((Wd @ H) * Wd).sum())


def main():
    torch.manual_seed(180)
    layer = torch.nn.Linear(256, 48).float()
    g = torch.Generator().manual_seed(181)
    sig = torch.exp(torch.randn(256, generator=g) * 0.5)
    xs = [(torch.randn(1, 320, 256, generator=g) * sig).half().float() for _ in range(2)]  # fp16 values: stored as fp16
    for x in xs:
        x[..., DEAD] = 0.0
    W = layer.weight.detach().clone()
    rms = float(W.pow(2).mean().sqrt())
    W_cs = [W + s * rms * torch.randn(W.shape, generator=g) for s in SIGMAS]

    est = LayerErrorEstimator(layer)
    for x in xs:
        est.update(x)
    est.pre_step()
    with torch.no_grad():
        vals = [est.estimate(w) for w in W_cs]
    ref64 = [fp64_estimate(xs, W, w) for w in W_cs]
    rel = [abs(v - r) / abs(r) for v, r in zip(vals, ref64)]
    out = os.path.join(HERE, "G18_errest.npz")
    np.savez_compressed(
        out, inputs=torch.stack(xs).half().numpy(), W=W.numpy(), W_c=torch.stack(W_cs).numpy(), H=est.H.numpy(),
        errors=np.array(vals, np.float64), rel_dist=np.array(rel, np.float64), dead=np.int64(DEAD),
        sigmas=np.array(SIGMAS, np.float64),
        meta=np.array(f"torch {torch.__version__} CPU fp32; evopress/src/error_estimator.py LayerErrorEstimator; "
                      f"nn.Linear(256, 48) seed 180, inputs seed 181, dead channel {DEAD}; rel_dist = |reference - fp64| / fp64: "
                      + " ".join(f"{r:.3e}" for r in rel)))
    print(f"errors {vals}  fp64 {ref64}  rel_dist {rel}  -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
