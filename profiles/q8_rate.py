"""Q8_0 on the GPU: decode, encode, switch and converter figures, one JSON line per part.  One process, HIP events around each
launch, warm-up first, the candidates ALTERNATING (every candidate takes every place in the order), median of N with min-max.
  decode    gq_dequantize_blocks(Q8_0) -> fp16 beside gq_dequantize_blocks(Q6_K) -> fp16 at 4096 x 14336 and 128256 x 4096
            (random block bytes with finite fp16 fields: the decode does not depend on the values)
  encode    gq_quantize_q8_0 at 128256 x 4096 from bf16 and from fp32, and the host clock of gguf_writer.quantize_q8_0 on the
            same tensor (one call; the function is the parent commit's)
  switch    a K-quant-only job list of a Llama-3-8B's 224 Linears (types cycling Q2_K..Q6_K, bf16 destinations) through this
            build's gq_level_switch and through a second library given with --parent-so (the parent commit's build)
  converter convert(outtype="q8_0") of a checkpoint that holds Llama-3-8B's token_embd, output and output_norm in bf16 (what
            the type rule sends to Q8_0 once every Linear of the blocks is a GPTQ result), written under --converter DIR:
            pipelined=True (the GPU producer) against pipelined=False (the host path: what the parent does for these tensors
            in either mode)
Bytes are algorithmic: every input read once, every output written once.
usage: python profiles/q8_rate.py [N=15] [--parent-so PATH] [--converter DIR] [--no-host]   (GPU box; needs only the built tree)"""
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from gptq_gguf_toolkit_amd import _cabi, ops  # noqa: E402

HBM_PEAK = 8.0e12
TS = {10: 84, 11: 110, 12: 144, 13: 176, 14: 210}
D_AT = {8: (0,), 10: (80, 82), 11: (108,), 12: (0, 2), 13: (0, 2), 14: (208,)}
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(argv[0]) if argv and argv[0].isdecimal() else 15


def flag(name):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None


def random_packed(t, R, C):
    bs, ts = (32, 34) if t == 8 else (256, TS[t])
    b = torch.randint(0, 256, (R * (C // bs), ts), dtype=torch.uint8, device="cuda")
    for off in D_AT[t]:  # exponent 31 -> 30: finite d / dmin
        hi = b[:, off + 1]
        hi[(hi & 0x7C) == 0x7C] &= 0xFB
    return b.view(R, -1)


def measure(cands):
    for fn in cands.values():
        for _ in range(3):
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
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def rate(t3, nbytes, params):
    med, lo, hi = t3
    return {"us": round(med * 1e6, 1), "min_us": round(lo * 1e6, 1), "max_us": round(hi * 1e6, 1),
            "bytes_per_param": round(nbytes / params, 4), "TBps": round(nbytes / med / 1e12, 3),
            "of_hbm_peak": round(nbytes / med / HBM_PEAK, 3)}


def decode():
    rows = []
    for R, C in ((4096, 14336), (128256, 4096)):
        q8, q6 = random_packed(8, R, C), random_packed(14, R, C)
        out = torch.empty(R, C, dtype=torch.float16, device="cuda")
        L, vp = _cabi.lib(), ctypes.c_void_p
        st = vp(torch.cuda.current_stream().cuda_stream)

        def run(t, src):
            _cabi.check(L.gq_dequantize_blocks(t, vp(src.data_ptr()), R, C, vp(0), vp(out.data_ptr()), _cabi.F16, st), "decode")

        m = measure({"q8_0": lambda: run(8, q8), "q6_k": lambda: run(14, q6)})
        rows.append({"R": R, "C": C, "q8_0": rate(m["q8_0"], q8.numel() + 2 * R * C, R * C),
                     "q6_k": rate(m["q6_k"], q6.numel() + 2 * R * C, R * C)})
        del q8, q6, out
    print(json.dumps({"part": "decode_to_fp16", "launches": N, "hbm_peak_TBps": HBM_PEAK / 1e12, "shapes": rows}), flush=True)


def encode():
    R, C = 128256, 4096
    torch.manual_seed(0)
    x32 = torch.randn(R, C, device="cuda") * 0.02
    xbf = x32.bfloat16()
    m = measure({"from_bf16": lambda: ops.quantize_q8_0(xbf), "from_fp32": lambda: ops.quantize_q8_0(x32)})
    nout = R * C // 32 * 34
    row = {"part": "encode", "launches": N, "R": R, "C": C, "from_bf16": rate(m["from_bf16"], 2 * R * C + nout, R * C),
           "from_fp32": rate(m["from_fp32"], 4 * R * C + nout, R * C)}
    if "--no-host" not in sys.argv:
        from gptq_gguf_toolkit_amd.gguf_writer import quantize_q8_0
        host = xbf.float().cpu().numpy()
        got = ops.quantize_q8_0(xbf).cpu().numpy()
        t0 = time.perf_counter()
        want = quantize_q8_0(host)
        row["host_numpy_s"] = round(time.perf_counter() - t0, 2)
        row["bytes_equal_to_host"] = bool((got == want).all())
    print(json.dumps(row), flush=True)


def switch(parent_so):
    block = [(4096, 4096), (1024, 4096), (1024, 4096), (4096, 4096), (14336, 4096), (14336, 4096), (4096, 14336)]
    shapes = block * 32
    types = [10 + i % 5 for i in range(len(shapes))]
    srcs = [random_packed(t, R, C).view(-1) for t, (R, C) in zip(types, shapes)]
    dsts = [torch.empty(R, C, dtype=torch.bfloat16, device="cuda") for R, C in shapes]
    nbytes = sum(s.numel() for s in srcs) + sum(d.numel() * 2 for d in dsts)
    table = (_cabi.SwitchJob * len(shapes))(*[_cabi.SwitchJob(s.data_ptr(), d.data_ptr(), None, d.shape[0], d.shape[1], t, _cabi.BF16)
                                              for s, d, t in zip(srcs, dsts, types)])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    libs = {"this": _cabi.lib()}
    if parent_so:
        P = ctypes.CDLL(parent_so)
        P.gq_level_switch.argtypes = [ctypes.POINTER(_cabi.SwitchJob), ctypes.c_int, ctypes.c_void_p]
        libs["parent"] = P

    def call(L):
        rc = L.gq_level_switch(table, len(shapes), st)
        assert rc == 0, rc

    call(libs["this"])
    torch.cuda.synchronize()
    got = [d.clone() for d in dsts[:7]]
    if parent_so:
        for d in dsts[:7]:
            d.zero_()
        call(libs["parent"])
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(got, dsts))
    m = measure({k: (lambda L=L: call(L)) for k, L in libs.items()})
    row = {"part": "switch_kquant_llama3_8b_224", "launches": N, "MB": round(nbytes / 1e6, 1)}
    for k, t3 in m.items():
        row[k] = rate(t3, nbytes, sum(d.numel() for d in dsts))
    if parent_so:
        row["this_over_parent"] = round(m["this"][0] / m["parent"][0], 4)
    print(json.dumps(row), flush=True)


def converter(work):
    from pathlib import Path
    from safetensors.torch import save_file
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import convert
    work = Path(work)
    hf = work / "hf"
    hf.mkdir(parents=True, exist_ok=True)
    V, h = 128256, 4096
    g = torch.Generator().manual_seed(0)
    sd = {"model.embed_tokens.weight": (torch.randn(V, h, generator=g) * 0.02).bfloat16(),
          "model.norm.weight": torch.ones(h, dtype=torch.bfloat16),
          "lm_head.weight": (torch.randn(V, h, generator=g) * 0.02).bfloat16()}
    save_file(sd, str(hf / "model.safetensors"))
    del sd
    (hf / "config.json").write_text(json.dumps({
        "architectures": ["LlamaForCausalLM"], "hidden_size": h, "intermediate_size": 14336, "num_hidden_layers": 32,
        "num_attention_heads": 32, "num_key_value_heads": 8, "vocab_size": V, "max_position_embeddings": 8192,
        "rms_norm_eps": 1e-5, "rope_theta": 500000.0}))
    (work / "q").mkdir(exist_ok=True)
    row = {"part": "converter_q8_0_embed_output", "values": 2 * V * h}
    for key, pipelined in (("warm_up", True), ("gpu_producer_s", True), ("host_path_s", False), ("gpu_producer_again_s", True)):
        tm = {}
        t0 = time.perf_counter()
        convert(hf, work / "q", work / f"{key}.gguf", "q8_0", vocab=False, pipelined=pipelined, timing=tm)
        row[key] = round(time.perf_counter() - t0, 2)
        row[key + "_stages"] = {k: round(v, 2) for k, v in tm.items()}
    a, b = (work / "gpu_producer_s.gguf").read_bytes(), (work / "host_path_s.gguf").read_bytes()
    row["files_equal"] = a == b
    for f in work.glob("*.gguf"):
        f.unlink()
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    decode()
    encode()
    switch(flag("--parent-so"))
    if flag("--converter"):
        converter(flag("--converter"))
