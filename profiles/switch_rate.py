"""K18 level-switch rates on the GPU, one JSON line.  One process, HIP events around each candidate, warm-up first, the
candidates ALTERNATING (every candidate takes every place in the order), median of N:
  batched : ONE gq_level_switch over the job list                          (what LevelStore.switch issues)
  a       : one gq_dequantize_blocks launch per job, back to back          (the same decode, launched per matrix)
  b       : torch.load(file, map_location=device).to(dtype) per job        (the reference's load_layers, files in a warm
            page cache; wall clock around a synchronised region, only with --files DIR: it writes the dense levels there)
Job lists: 12 mixed Q2_K..Q6_K jobs at 4096 x 14336, 12 at 4096 x 4096, and the 224 Linears of a Llama-3-8B (32 blocks of
q, k, v, o, gate, up, down at their shapes), the types cycling over the list.  Sources are random bytes with finite fp16
fields (the decode does not depend on the values); destinations bf16.  Bytes are algorithmic: packed bytes in, 2 B/param out.
usage: python profiles/switch_rate.py [N=15] [--files DIR]   (GPU box; needs only the built tree)"""
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from gptq_gguf_toolkit_amd import _cabi, ops  # noqa: E402

TS = {10: 84, 11: 110, 12: 144, 13: 176, 14: 210}
D_AT = {10: (80, 82), 11: (108,), 12: (0, 2), 13: (0, 2), 14: (208,)}
HBM_PEAK = 8.0e12
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(argv[0]) if argv else 15
FILES = sys.argv[sys.argv.index("--files") + 1] if "--files" in sys.argv else None


def random_packed(t, R, C):
    b = torch.randint(0, 256, (R * (C // 256), TS[t]), dtype=torch.uint8, device="cuda")
    for off in D_AT[t]:  # exponent 31 -> 30: finite d / dmin
        hi = b[:, off + 1]
        hi[(hi & 0x7C) == 0x7C] &= 0xFB
    return b.view(-1)


def measure(cands):
    for fn in cands.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times, keys = {k: [] for k in cands}, list(cands)
    for it in range(N):
        evs = []
        for k in keys[it % len(keys):] + keys[:it % len(keys)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cands[k]()
            e1.record()
            evs.append((k, e0, e1))
        torch.cuda.synchronize()
        for k, e0, e1 in evs:
            times[k].append(e0.elapsed_time(e1) * 1e-3)
    return {k: statistics.median(v) for k, v in times.items()}, {k: (min(v), max(v)) for k, v in times.items()}


def case(name, shapes):
    L, vp = _cabi.lib(), ctypes.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)
    types = [10 + i % 5 for i in range(len(shapes))]
    srcs = [random_packed(t, R, C) for t, (R, C) in zip(types, shapes)]
    dsts = [torch.empty(R, C, dtype=torch.bfloat16, device="cuda") for R, C in shapes]
    jobs = [(s, d, t, None) for s, d, t in zip(srcs, dsts, types)]
    nbytes = sum(s.numel() for s in srcs) + sum(d.numel() * 2 for d in dsts)

    def batched():
        ops.level_switch(jobs)

    def per_matrix():
        for s, d, t in zip(srcs, dsts, types):
            _cabi.check(L.gq_dequantize_blocks(t, vp(s.data_ptr()), d.shape[0], d.shape[1], vp(0), vp(d.data_ptr()), _cabi.BF16, st),
                        "gq_dequantize_blocks")

    batched()
    got = [d.clone() for d in dsts[:5]]
    for d in dsts[:5]:
        d.zero_()
    per_matrix()
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(got, dsts))
    med, rng = measure({"batched": batched, "a_per_matrix": per_matrix})
    row = {"case": name, "jobs": len(jobs), "MB": round(nbytes / 1e6, 1)}
    for k in med:
        row[k] = {"us": round(med[k] * 1e6, 1), "min_us": round(rng[k][0] * 1e6, 1), "max_us": round(rng[k][1] * 1e6, 1),
                  "TBps": round(nbytes / med[k] / 1e12, 3), "of_hbm_peak": round(nbytes / med[k] / HBM_PEAK, 3)}
    row["batched_over_a"] = round(med["batched"] / med["a_per_matrix"], 4)
    if FILES and len(jobs) <= 12:
        os.makedirs(FILES, exist_ok=True)
        paths = []
        for i, d in enumerate(dsts):
            paths.append(os.path.join(FILES, f"{name}_{i}.pth"))
            torch.save(d.half().cpu(), paths[-1])
        layers = [torch.nn.Linear(d.shape[1], d.shape[0], bias=False, dtype=torch.bfloat16, device="cuda") for d in dsts]
        walls = []
        for _ in range(4):  # the first pass warms the page cache
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p, layer in zip(paths, layers):
                layer.weight.data = torch.load(p, map_location=layer.weight.device).to(layer.weight.dtype)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        row["b_torch_load_to"] = {"ms": round(statistics.median(walls[1:]) * 1e3, 2), "file_MB": round(sum(os.path.getsize(p) for p in paths) / 1e6, 1)}
        for p in paths:
            os.remove(p)
    return row


def main():
    block = [(4096, 4096), (1024, 4096), (1024, 4096), (4096, 4096), (14336, 4096), (14336, 4096), (4096, 14336)]
    res = {"launches": N, "hbm_peak_TBps": HBM_PEAK / 1e12, "cases": [
        case("12x4096x14336", [(4096, 14336)] * 12), case("12x4096x4096", [(4096, 4096)] * 12), case("llama3_8b_224", block * 32)]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
