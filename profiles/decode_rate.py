"""K15 decode rates on the GPU, one JSON line.  At 4096 x 14336 Q4_K and 128256 x 4096 Q6_K (fields from ops.rtn_quantize), in
one process, HIP events around each launch, warm-up first, the candidates ALTERNATING, median of N launches each:
  (a) gq_dequantize_blocks -> fp16                       (the fused decode)
  (b) gq_unpack + gq_dequantize -> fp16, back to back    (what (a) replaces)
  (c) gq_pack alone, gq_dequantize alone                 (the neighbouring streaming kernels: the yardstick of this class)
Rates are algorithmic bytes from the shapes (every input read once, every output written once) over the median time; the
smaller shape's 117 MB of fp16 output fits the 256 MiB Infinity Cache, the larger one's 1 GB does not.
A second part ("iq4") times (a) alone at 4096 x 14336 for Q4_K, IQ4_XS and IQ4_NL in the same alternating way: the two types
that are only read (random blocks, profiles/iq4_blocks.py) beside the nearest K-quant.
usage: python profiles/decode_rate.py [N=25]   (GPU box; needs only the built tree)"""
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from gptq_gguf_toolkit_amd import _cabi, ops  # noqa: E402
from iq4_blocks import iq4_blocks  # noqa: E402

HBM_PEAK = 8.0e12
TS = {12: 144, 14: 210}
NAME = {12: "Q4_K", 14: "Q6_K"}
N = int(sys.argv[1]) if len(sys.argv) > 1 else 25


def main():
    L, vp = _cabi.lib(), ctypes.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)
    p = lambda t: vp(t.data_ptr())  # noqa: E731
    res = {"launches": N, "hbm_peak_TBps": HBM_PEAK / 1e12, "shapes": []}
    for t, R, C in ((12, 4096, 14336), (14, 128256, 4096)):
        torch.manual_seed(0)
        W = (torch.randn(R, C, device="cuda") * 0.02).half()
        q, d, s, dmin, m = ops.rtn_quantize(W, t)
        del W
        packed = ops.pack(t, q, d, s, dmin, m)
        out = torch.empty(R, C, dtype=torch.float16, device="cuda")
        q2, d2, s2, dmin2, m2 = [torch.empty_like(x) for x in (q, d, s, dmin, m)]
        packed2 = torch.empty_like(packed)
        G = 32 if t == 12 else 16
        aux = R * (C // 256) * 4 + 2 * R * (C // G)  # d, dmin fp16 + s, m bytes
        nblk = R * (C // 256) * TS[t]

        def fused():
            _cabi.check(L.gq_dequantize_blocks(t, p(packed), R, C, vp(0), p(out), _cabi.F16, st), "gq_dequantize_blocks")

        def unpack():
            _cabi.check(L.gq_unpack(t, p(packed), R, C, p(q2), p(d2), p(s2), p(dmin2), p(m2), st), "gq_unpack")

        def deq():
            _cabi.check(L.gq_dequantize(t, p(q), p(d), p(s), p(dmin), p(m), R, C, p(out), _cabi.F16, st), "gq_dequantize")

        def two():
            unpack()
            _cabi.check(L.gq_dequantize(t, p(q2), p(d2), p(s2), p(dmin2), p(m2), R, C, p(out), _cabi.F16, st), "gq_dequantize")

        def pack():
            _cabi.check(L.gq_pack(t, p(q), p(d), p(s), p(dmin), p(m), R, C, p(packed2), st), "gq_pack")

        cands = {"a_dequantize_blocks": (fused, nblk + 2 * R * C), "b_unpack_then_dequantize": (two, nblk + 2 * (R * C + aux) + 2 * R * C),
                 "c_pack": (pack, R * C + aux + nblk), "c_dequantize": (deq, R * C + aux + 2 * R * C), "unpack": (unpack, nblk + R * C + aux)}
        for fn, _ in cands.values():  # warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in cands}
        keys = list(cands)
        for it in range(N):
            evs = []
            for k in keys[it % len(keys):] + keys[:it % len(keys)]:  # every candidate takes every place in the order
                fn = cands[k][0]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                evs.append((k, e0, e1))
            torch.cuda.synchronize()
            for k, e0, e1 in evs:
                times[k].append(e0.elapsed_time(e1) * 1e-3)
        assert torch.equal(q2.view(torch.uint8), q.view(torch.uint8)) and torch.equal(packed2, packed)
        row = {"q_type": NAME[t], "R": R, "C": C}
        for k, (_, nbytes) in cands.items():
            med = statistics.median(times[k])
            row[k] = {"us": round(med * 1e6, 1), "bytes_per_param": round(nbytes / (R * C), 3), "TBps": round(nbytes / med / 1e12, 3),
                      "of_hbm_peak": round(nbytes / med / HBM_PEAK, 3)}
        row["a_faster_than_b"] = row["a_dequantize_blocks"]["us"] < row["b_unpack_then_dequantize"]["us"]
        res["shapes"].append(row)
    res["iq4"] = iq4_rows()
    print(json.dumps(res))


def iq4_rows(R=4096, C=14336):
    g = torch.Generator(device="cuda").manual_seed(0)
    W = torch.randn(R, C, device="cuda", generator=g) * 0.02
    src = {"Q4_K": (12, ops.pack(12, *ops.rtn_quantize(W, 12))), "IQ4_XS": (23, iq4_blocks(23, R, C, g)),
           "IQ4_NL": (20, iq4_blocks(20, R, C, g))}
    del W
    for t, blocks in src.values():  # warm-up
        for _ in range(3):
            ops.dequantize_blocks(t, blocks, torch.float16)
    torch.cuda.synchronize()
    times, keys = {k: [] for k in src}, list(src)
    for it in range(N):
        evs = []
        for k in keys[it % len(keys):] + keys[:it % len(keys)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.dequantize_blocks(src[k][0], src[k][1], torch.float16)
            e1.record()
            evs.append((k, e0, e1))
        torch.cuda.synchronize()
        for k, e0, e1 in evs:
            times[k].append(e0.elapsed_time(e1) * 1e-3)
    rows = {"R": R, "C": C, "out": "fp16 (each call allocates its output)"}
    for k, (t, blocks) in src.items():
        med, nbytes = statistics.median(times[k]), blocks.numel() + 2 * R * C
        rows[k] = {"us": round(med * 1e6, 1), "bytes_per_param": round(nbytes / (R * C), 3), "TBps": round(nbytes / med / 1e12, 3)}
    for k in ("IQ4_XS", "IQ4_NL"):
        rows[k]["over_Q4_K"] = round(rows[k]["us"] / rows["Q4_K"]["us"], 3)
    return rows


if __name__ == "__main__":
    main()
