"""Round 6 GPU tests (VERDICT r05 "next round" items)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from gptq_gguf_toolkit_amd import ops as O
    return O


def _hessian(C, seed, T=None):
    torch.manual_seed(seed)
    T = T or 2 * C
    X = (torch.randn(T, C, device="cuda") * torch.exp(torch.randn(C, device="cuda") * 0.5)).half()
    H = torch.zeros(C, C, device="cuda")
    from gptq_gguf_toolkit_amd import ops as O
    O.h_accumulate(H, X, 0.0, 2.0 / 4)
    return H


# ----------------------------------------------------------------- item 3: the reference-side binding, executed as printed
def _integration_stub():
    import re
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lvl2 = doc[doc.index("## Level 2"):]
    m = re.search(r"```python\n(.*?)```", lvl2, re.S)
    assert m, "INTEGRATION.md no longer shows the Level-2 ctypes stub"
    return m.group(1)


def test_integration_stub_runs_as_printed():
    """the ctypes stub INTEGRATION.md tells a maintainer of the reference to paste into src/gptq.py is
    extracted from the file and exec'd verbatim (only GPTQGGUF_HIP_SO names where the library lies), then drives
    GPTQ.update -> GPTQ._prepare -> GPTQ.step through it on the reference's own vectors: G4 Hessians (fp32 accumulation-order
    tolerance), G5 U (factorisation tolerance), G6 integers / scales and G7 packed bytes bit for bit.  A stale ABI version or
    a drifted argtypes list fails here."""
    import numpy as np
    from conftest import load_golden, triu_unpack
    from gptq_gguf_toolkit_amd import SO_PATH, ops
    os.environ["GPTQGGUF_HIP_SO"] = SO_PATH
    ns = {}
    exec(compile(_integration_stub(), "INTEGRATION.md:Level-2", "exec"), ns)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    # GPTQ.update (gptq.py:96,108-112)
    g = load_golden("g4_g5_hessian")
    for tag, dt in (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)):
        X = g[f"X_{tag}"]
        C = X.shape[-1]
        H = torch.zeros(C, C, device="cuda")
        for n, xb in enumerate(X):
            ns["h_addmm_"](H, dev(xb).to(dt), n / (n + 1), 2.0 / (n + 1))
        ref = g[f"H_{tag}"]
        assert np.abs(H.cpu().numpy() - ref).max() <= 3e-6 * np.abs(ref).max(), tag
    # GPTQ._prepare (gptq.py:304-324)
    H, W = dev(g["prep_H_in"]), dev(g["prep_W_in"])
    U, flag = ns["prepare"](H, W, 0.01)
    assert int(flag.item()) == 0 and np.array_equal(W.cpu().numpy(), g["prep_W_after_prestep"])
    Uref = triu_unpack(g["prep_U_triu"], H.shape[0])
    assert np.abs(U.cpu().numpy() - Uref).max() <= 2e-4 * np.abs(Uref).max()
    # GPTQ.step (gptq.py:158-276): the reference's integers
    g6 = load_golden("g6_g7_step_and_pack")
    tags = sorted({k.rsplit("_", 1)[0] for k in g6.files if k.endswith("_q") and "mklsqrt" not in k and "_b128_s0" in k})
    assert len(tags) >= 5
    types = {"Q2_K": 10, "Q3_K": 11, "Q4_K": 12, "Q5_K": 13, "Q6_K": 14}
    for tag in tags:
        case, n1, n2, b, s_ = tag.split("_")
        name = f"{n1}_{n2}"
        W0 = g6[f"{case}_W0"]
        R, C = W0.shape
        U = dev(triu_unpack(g6[f"{case}_U_triu"], C))
        W = dev(W0)
        G = {"Q2_K": 16, "Q3_K": 16, "Q4_K": 32, "Q5_K": 32, "Q6_K": 16}[name]  # quant_utils.py:19-26
        signed = name in ("Q3_K", "Q6_K")
        q = torch.empty(R, C, dtype=torch.int8 if signed else torch.uint8, device="cuda")
        d = torch.empty(R, C // 256, dtype=torch.float16, device="cuda")
        dmin = torch.empty_like(d)
        s = torch.empty(R, C // G, dtype=torch.int8 if signed else torch.uint8, device="cuda")
        m = torch.empty_like(s)
        ns["step"](W, U, types[name], int(b[1:]), False, -1.0, 0.1, 20, "absmax", q, d, s, dmin, m)
        torch.cuda.synchronize()
        assert np.array_equal(q.cpu().numpy(), g6[f"{tag}_q"]), tag
        assert np.array_equal(d.cpu().view(torch.int16).numpy().view(np.uint16), g6[f"{tag}_d"]), tag
        assert np.array_equal(s.cpu().numpy(), g6[f"{tag}_s"]) and np.array_equal(m.cpu().numpy(), g6[f"{tag}_m"]), tag
        if f"{tag}_packed" in g6.files:
            assert np.array_equal(ops.pack(types[name], q, d, s, dmin, m).cpu().numpy(), g6[f"{tag}_packed"]), tag


# ----------------------------------------------------------------- item 7: the default line at 8 ranks, whole-model leg included
def test_default_workload_at_eight_ranks_with_the_whole_model_leg():
    """the first real 8-GPU lease must not run a code path for the first time.  The driver's command form
    (`python3 bench.py --gpus 8 ...`) on the DEFAULT workload (llama3-8b-block-q4k: calibration shards, one collective per
    distinct Hessian, LPT owners, the row-split down_proj, ONE all-gather per block) with 16 calibration sequences, INCLUDING
    the whole-model leg (2 layers: Quantizer.quantize with sharded calibration, collectives inside the forward cadence, data.pth
    files dealt to the ranks) -- 8 ranks share the GPU over gloo when the box has fewer than 8."""
    n = 8
    backend = [] if torch.cuda.device_count() >= n else ["--backend", "gloo"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), *backend, "--steps", "1", "--warmup", "1",
           "--calib-seqs", "16", "--layers", "2", "--full"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2
    full, compact = lines
    assert full["n_gpus"] == n and full["ranks_seen"] == n and full["value"] > 0
    assert full["config"]["calib_seqs_per_rank"] == 2 and "llama3-8b-block-q4k" in full["config"]["workload"]
    coll = full["collectives_per_step"]
    assert coll["all_gather"] == 1 and coll["broadcast"] == 0 and coll["all_reduce"] + coll["reduce"] == 4  # one per distinct H
    for key in ("whole_model", "whole_model_hf_eager", "whole_model_batch4"):
        wm = full[key]
        assert "error" not in wm, wm
        assert wm["wall_s_quantizer_region"] > 0 and wm["data_pth"]["files"] == 2 * 7 + 2  # 2 blocks x 7 Linears + embed + lm_head
        assert wm["end_to_end_gguf"] is None  # the packer leg belongs to the N = 1 line
    assert compact["whole_model_wall_s"] == full["whole_model"]["wall_s_quantizer_region"] and compact["cpu_baseline"] is None
    assert "Connection closed" not in json.dumps(full)


# ----------------------------------------------------------------- item 2: the .gguf file decodes to the quantized model
def test_gguf_file_of_an_8b_width_model_decodes_to_the_written_back_weights(tmp_path):
    """VERDICT r05 next #2, the parity side of the end-to-end leg (a size-independent property at the BASELINE width): quantize a
    2-block random-init Llama-3-8B-shaped model (hidden 4096, intermediate 14336, GQA 32 / 8, Q4_K everywhere incl. embed / lm_head),
    pack it with the pipelined converter, then decode EVERY quantized tensor of the .gguf with the independent ggml-layout decoder
    (tests/ggml_spec.py) and dequantize it by ggml's formula (d sc q - dmin m, fp32): after the cast to the model dtype it must
    equal, bit for bit, the weight the quantizer wrote back into the live model (quantizer.py:257-264) -- q / k rows through the
    converter's un-permute (:320-324).  The tensor-by-tensor flow writes the same bytes."""
    import importlib.util
    import numpy as np
    from pathlib import Path
    from ggml_spec import unpack
    from gptq_gguf_toolkit_amd.gguf_writer import read_gguf
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import convert, map_tensor_name, permute
    from gptq_gguf_toolkit_amd.quantizer import Quantizer
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    dev = torch.device("cuda:0")
    wl = B.WORKLOADS["llama3-8b-model-q4k"]
    cfg = dict(wl["model"])
    cfg["num_hidden_layers"] = 2
    model = B.build_model(cfg, dev)
    hf, sd = tmp_path / "hf", tmp_path / "q"
    model.save_pretrained(str(hf), safe_serialization=True)
    g = torch.Generator().manual_seed(3)
    data = [([], {"input_ids": torch.randint(0, cfg["vocab_size"], (1, 1024), generator=g)}) for _ in range(8)]
    q4 = B.QT["Q4_K"]
    qc = {k: q4 for k in ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "down_proj", "up_proj", "embed_tokens", "lm_head")}
    Quantizer(model, data_loader=data, quantizable_modules=r".*layers.*((q|k|v|o|gate|up|down)_proj)$",
              quantizer_kwargs=dict(B.QUANTIZER_KW, verbose=False), pre_block_modules=["model.embed_tokens"], block_modules="model.layers",
              post_block_modules=["lm_head"], quant_non_block_modules=True, device=str(dev), save_dir=str(sd)).quantize(qc)
    torch.cuda.synchronize()
    out = convert(Path(hf), Path(sd), tmp_path / "m.gguf", "f16", vocab=False)
    convert(Path(hf), Path(sd), tmp_path / "m_flow.gguf", "f16", vocab=False, pipelined=False)
    import hashlib
    sha = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()  # noqa: E731
    assert sha(out) == sha(tmp_path / "m_flow.gguf")
    kv, ts = read_gguf(str(out))
    assert kv["llama.block_count"] == 2 and kv["llama.embedding_length"] == 4096
    n_head, n_kv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    checked = 0
    for name, w in model.state_dict().items():
        if w.dim() != 2:
            continue
        shape, gt, raw = ts[map_tensor_name(name)]
        assert gt == 12 and shape == tuple(w.shape), name  # Q4_K bytes
        codes, d, sc, dmin, mn = unpack(gt, raw.reshape(shape[0], -1))
        f16 = lambda bits: torch.from_numpy(bits.astype(np.uint16).view(np.int16).copy()).view(torch.float16).float()  # noqa: E731
        ds = (f16(d).repeat_interleave(8, dim=1) * torch.from_numpy(sc.astype(np.float32)))        # [R, C / 32]
        dm = (f16(dmin).repeat_interleave(8, dim=1) * torch.from_numpy(mn.astype(np.float32)))
        deq = ds.repeat_interleave(32, dim=1) * torch.from_numpy(codes.astype(np.float32)) - dm.repeat_interleave(32, dim=1)
        want = w.detach().cpu()
        if name.endswith("q_proj.weight"):
            want = permute(want, n_head, n_head)
        elif name.endswith("k_proj.weight"):
            want = permute(want, n_head, n_kv)
        assert torch.equal(deq.to(want.dtype), want), f"{name}: {(deq.to(want.dtype) != want).float().mean().item():.3%} of the weights differ"
        checked += 1
    assert checked == 2 * 7 + 2
    norm = ts["blk.1.ffn_norm.weight"]
    assert norm[1] == 0 and norm[0] == (4096,)  # 1-D stays F32
