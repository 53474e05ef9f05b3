#!/usr/bin/env python3
"""Widest chain alone: gq_h_prepare(14336) and the column loop of 4096 x 14336 Q4_K, each timed sync to sync."""
import json, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gptq_gguf_toolkit_amd import ops, _cabi
Q4_K = 12
R, C, N = 4096, 14336, int(os.environ.get("N", 10))
torch.manual_seed(0)
T = 2 * C
X = (torch.randn(T, C, device="cuda") * torch.exp(torch.randn(C, device="cuda") * 0.5)).half()
H0 = torch.zeros(C, C, device="cuda")
ops.h_accumulate(H0, X, 0.0, 2.0 / 8)
del X
W0 = torch.randn(R, C, device="cuda") * 0.02
_cabi.prof_enable([])
prep, loop = [], []
for it in range(N + 2):
    H = H0.clone(); W = W0.clone(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    U, flag = ops.h_prepare(H, W, 0.01)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    out = ops.gptq_quantize(W, U, Q4_K, 128)
    torch.cuda.synchronize(); t2 = time.perf_counter()
    if it >= 2:
        prep.append(1e3 * (t1 - t0)); loop.append(1e3 * (t2 - t1))
import zlib
crc = zlib.crc32(U.cpu().numpy().tobytes()) ^ zlib.crc32(out[0].cpu().numpy().tobytes())
print(json.dumps({"tag": os.environ.get("TAG"), "prep_min": round(min(prep), 3), "prep_med": round(statistics.median(prep), 3),
                  "loop_min": round(min(loop), 3), "loop_med": round(statistics.median(loop), 3), "flag": int(flag.item()),
                  "helper": bool(ops.uses_helper_stream(R, C, 128)), "crc": crc}))
