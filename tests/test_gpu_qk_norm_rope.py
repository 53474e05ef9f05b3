"""-m gpu: K32 -- gq_fwd_qk_norm_rope (csrc/forward/gq_qk_norm_rope.hip) against the eager torch expressions it replaces
(transformers' Qwen3RMSNorm over head_dim on q and k, then apply_rotary_pos_emb), Qwen3Attention.forward under
fused_forward("exact"), and a tiny Qwen3 end to end: quantize, convert, load, ppleval, level database, stitch, generate.

Tolerances: the kernel is bit-identical or not used -- torch.equal on both outputs and on the fp32 statistics against torch's
own mean and rsqrt.  ppleval's ln ppl of the packed-resident and of the dense-resident load: the rule of
tests/test_gpu_packed_vocab.py::test_ppleval_packed_vocab -- floor = max |dense 16-bit logits - the same weights' fp32 logits|,
packed logits within 2 floor of fp32, ln ppl 2-Lipschitz in the logits (stated where it is asserted)."""
import copy
import ctypes
import io
import json
import math
import os
import sys
from contextlib import redirect_stdout
from pathlib import Path

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import tiny_qwen3 as TQ  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(1, 8, 4, 2), (2, 33, 8, 2), (1, 2048, 32, 8)]  # few rows; odd rows, cos of batch 1 expanded to 2; Qwen3-8B's heads
GUARD = 64  # bytes either side of an output
EPS = 1e-6


def _inputs(B, L, Hq, Hk, D, dtype, cos_batch=None):
    """q, k with rows of zeros, a row with one huge value (its other elements' products with 1 / rms are subnormal in the
    dtype), norm weights, and a rotary table.  cos_batch 1: [1, L, D], as a model hands it over for any batch."""
    g = torch.Generator(device="cuda").manual_seed(1000 * D + 10 * L + Hq)
    q = torch.randn(B, L, Hq, D, device="cuda", generator=g) * torch.exp(torch.randn(D, device="cuda", generator=g))
    k = torch.randn(B, L, Hk, D, device="cuda", generator=g) * torch.exp(torch.randn(D, device="cuda", generator=g))
    huge, tiny = (6.0e4, 1.0e-3) if dtype == torch.float16 else (1.0e19, 1.0e-21)  # huge^2 is finite in fp32
    for x in (q, k):
        x[0, 0, 0] = 0.0
        x[-1, -1, -1] = 0.0
        x[0, L // 2, -1] = tiny
        x[0, L // 2, -1, D // 3] = huge
        x[-1, 1, 0] = -tiny
        x[-1, 1, 0, D - 1] = -huge
    q, k = q.to(dtype), k.to(dtype)
    wq = (1.0 + 0.3 * torch.randn(D, device="cuda", generator=g)).to(dtype)
    wk = (1.0 + 0.3 * torch.randn(D, device="cuda", generator=g)).to(dtype)
    inv = 1.0 / (1000000.0 ** (torch.arange(0, D, 2, device="cuda").float() / D))
    ang = torch.arange(L, device="cuda").float()[None, :, None] * inv[None, None, :]
    emb = torch.cat([ang, ang], -1).expand(cos_batch or B, L, D)
    return q, k, wq, wk, emb.cos().to(dtype).contiguous(), emb.sin().to(dtype).contiguous()


def _eager(q, k, wq, wk, cos, sin):
    """(q', k') in [B, L, H, D], fp32 var and rsqrt per row (q rows first): the installed transformers' own modules."""
    from transformers.models.qwen3 import modeling_qwen3 as M
    D = q.shape[-1]
    nq, nk = M.Qwen3RMSNorm(D, eps=EPS).to("cuda", q.dtype), M.Qwen3RMSNorm(D, eps=EPS).to("cuda", q.dtype)
    with torch.no_grad():
        nq.weight.copy_(wq)
        nk.weight.copy_(wk)
        wantq, wantk = M.apply_rotary_pos_emb(nq(q).transpose(1, 2), nk(k).transpose(1, 2), cos, sin)
        var = torch.cat([q.to(torch.float32).pow(2).mean(-1).reshape(-1), k.to(torch.float32).pow(2).mean(-1).reshape(-1)])
        r = torch.rsqrt(var + EPS)
    return wantq.transpose(1, 2), wantk.transpose(1, 2), var, r


def _guarded(like):
    """An output buffer with GUARD bytes of 0xA5 either side -> (whole uint8 buffer, the view the kernel writes)."""
    n = like.numel() * like.element_size()
    buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(like.dtype).view(like.shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("B,L,Hq,Hk", SHAPES)
def test_kernel_is_bit_identical_to_the_eager_ops(B, L, Hq, Hk, D, dtype):
    from gptq_gguf_toolkit_amd import ops
    q, k, wq, wk, cos, sin = _inputs(B, L, Hq, Hk, D, dtype, cos_batch=1 if B > 1 else None)
    wantq, wantk, var, r = _eager(q, k, wq, wk, cos, sin)
    c, s = cos.expand(B, L, D).contiguous(), sin.expand(B, L, D).contiguous()
    bq, oq = _guarded(q)
    bk, ok = _guarded(k)
    gq_, gk_, stats = ops.fwd_qk_norm_rope(q, k, wq, wk, c, s, EPS, want_stats=True, out=(oq, ok))
    torch.cuda.synchronize()
    assert gq_.data_ptr() == oq.data_ptr() and stats.shape == (B * L * (Hq + Hk), 2)
    # the fp32 statistics first: 16-bit outputs hide most differences of the summation order
    bad = int((stats[:, 0] != var).sum())
    assert bad == 0, f"mean(x^2) differs from torch's in {bad} of {var.numel()} rows"
    assert torch.equal(stats[:, 1], r)
    assert bool(torch.isfinite(wantq).all()) and bool(torch.isfinite(wantk).all())
    assert torch.equal(gq_, wantq) and torch.equal(gk_, wantk)
    assert _guards_intact(bq) and _guards_intact(bk)
    # the subnormal products are there and survive: elements of the huge-value rows that are subnormal in the dtype and not zero
    tiny = torch.finfo(dtype).tiny
    sub = (wantq.float().abs() < tiny) & (wantq != 0)
    assert bool(sub.any())
    # without stats: the same bits
    gq2, gk2 = ops.fwd_qk_norm_rope(q, k, wq, wk, c, s, EPS)
    assert torch.equal(gq2, wantq) and torch.equal(gk2, wantk)


def test_refusals_return_status_codes_and_launch_nothing():
    from gptq_gguf_toolkit_amd import _cabi, ops
    L_ = ops.lib()
    BAD_TYPE, BAD_SHAPE, E_NULL = -1, -2, -6  # include/gptq_gguf.h
    q, k, wq, wk, cos, sin = _inputs(1, 4, 2, 1, 64, torch.float16)
    bq, oq = _guarded(q)
    bk, ok = _guarded(k)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731

    def call(qp=None, head_dim=64, dtype=_cabi.F16, out=None):
        return L_.gq_fwd_qk_norm_rope(p(q) if qp is None else qp, p(k), p(wq), p(wk), p(cos), p(sin), p(oq) if out is None else out,
                                      p(ok), 4, 2, 1, head_dim, EPS, dtype, ctypes.c_void_p(0), st)

    assert call(head_dim=96) == BAD_SHAPE and b"head_dim=96" in L_.gq_last_error()
    assert call(qp=p(q, 2)) == BAD_SHAPE and call(out=p(oq, 8)) == BAD_SHAPE  # misaligned pointers
    assert call(dtype=_cabi.F32) == BAD_TYPE
    assert call(out=ctypes.c_void_p(0)) == E_NULL
    assert call(head_dim=32) == BAD_SHAPE and call(head_dim=512) == BAD_SHAPE
    torch.cuda.synchronize()
    assert bool((bq == 0xA5).all()) and bool((bk == 0xA5).all())  # nothing was launched: the outputs are untouched
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((oq.view(torch.uint8) == 0xA5).all()) and _guards_intact(bq) and _guards_intact(bk)
    with pytest.raises(_cabi.GQError):  # fp32 through the Python call: refused, no fallback
        ops.fwd_qk_norm_rope(*(t.float() for t in (q, k, wq, wk, cos, sin)), EPS)


def _attn_linears(model):
    return [(n, m) for n, m in model.named_modules() if n.endswith(("q_proj", "k_proj", "v_proj", "o_proj"))]


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_qwen3_under_the_exact_level(dtype, monkeypatch):
    """The logits of the SECOND call of an input class -- the call in which the kernel runs -- equal the unpatched model's;
    the hooks on the four attention Linears fire once per forward; a forward with a KV cache takes the original path."""
    from gptq_gguf_toolkit_amd import forward_fused, ops
    from transformers.models.qwen3 import modeling_qwen3 as M
    model = TQ.tiny_qwen3(dtype=dtype).cuda()
    ids = torch.randint(0, TQ.VOCAB, (2, 48), generator=torch.Generator().manual_seed(3)).cuda()
    calls, real = [], ops.fwd_qk_norm_rope

    def counted(*a, **kw):
        calls.append(kw.get("want_stats", False))
        return real(*a, **kw)

    monkeypatch.setattr(ops, "fwd_qk_norm_rope", counted)
    fired = {}
    hooks = [m.register_forward_pre_hook(lambda mod, args, n=n: fired.__setitem__(n, fired.get(n, 0) + 1))
             for n, m in _attn_linears(model)]
    assert len(hooks) == 4 * TQ.LAYERS
    original = M.Qwen3Attention.forward
    with torch.no_grad():
        want = model(input_ids=ids, use_cache=False).logits
        assert set(fired.values()) == {1}
        forward_fused.reset_verdicts()
        with forward_fused.fused_forward("exact") as patched:
            assert "Qwen3Attention.forward" in patched and M.Qwen3Attention.forward is not original
            first = model(input_ids=ids, use_cache=False).logits   # the eager expressions decide, and are what is returned
            # one class, which both layers share: layer 0 verifies it, layer 1 already runs the kernel
            assert calls == [True, False] and set(fired.values()) == {2}
            assert forward_fused._qkn_verdict and all(forward_fused._qkn_verdict.values())
            second = model(input_ids=ids, use_cache=False).logits  # the kernel runs, in both layers
            assert calls == [True, False, False, False] and set(fired.values()) == {3}
            # a forward with a KV cache: the original path, no launch of this kernel
            cached = model(input_ids=ids, use_cache=True)
            assert cached.past_key_values is not None and len(calls) == 4 and set(fired.values()) == {4}
            with torch.enable_grad():  # grad enabled: the original path as well
                model(input_ids=ids, use_cache=False)
            assert len(calls) == 4
        assert M.Qwen3Attention.forward is original
        forward_fused.reset_verdicts()
        assert not forward_fused._qkn_verdict
    for h in hooks:
        h.remove()
    assert torch.equal(first, want) and torch.equal(second, want)


# ------------------------------------------------------------------------------------------------ end to end
QUANT_KW = dict(rel_damp=0.01, block_size=128, act_order=False, quant_scale="absmax", static_groups=False, rmin=-1.0,
                rdelta=0.1, nstep=20, verbose=False)
MIXED = {"q_proj": "Q3_K", "k_proj": "Q2_K", "v_proj": "Q4_K", "o_proj": "Q5_K", "gate_proj": "Q6_K", "down_proj": "Q3_K",
         "up_proj": "Q4_K", "embed_tokens": "Q6_K", "lm_head": "Q6_K"}


def _load_hf(path, dtype=torch.float16):
    from transformers import AutoModelForCausalLM
    return AutoModelForCausalLM.from_pretrained(path, dtype=dtype, attn_implementation="eager").cuda().eval()


def _tree_bytes(save_dir):
    out = {}
    for d, _, fs in sorted(os.walk(save_dir)):
        for f in sorted(fs):
            out[os.path.relpath(os.path.join(d, f), save_dir)] = open(os.path.join(d, f), "rb").read()
    return out


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The tiny fp16 Qwen3 saved with a synthetic byte-level BPE tokenizer, quantized twice (fused_forward exact / off),
    converted to a .gguf with its vocabulary."""
    from gptq_gguf_toolkit_amd import forward_fused
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import convert
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    from gptq_gguf_toolkit_amd.quantizer import Quantizer
    tmp = tmp_path_factory.mktemp("qwen3")
    hf = tmp / "hf"
    TQ.tiny_qwen3(dtype=torch.float16).save_pretrained(str(hf), safe_serialization=True)
    TQ.write_bpe_tokenizer(hf)
    data = [([], {"input_ids": ids}) for ids in TQ.tiny_calib()]
    w = {"tmp": tmp, "hf": str(hf), "fused": {}, "verdicts": {}}
    for level in ("exact", "off"):
        model = _load_hf(str(hf))
        drv = Quantizer(model, data_loader=data, quantizable_modules=TQ.LINEARS, quantizer_kwargs=QUANT_KW,
                        pre_block_modules=["model.embed_tokens"], block_modules="model.layers", post_block_modules=["lm_head"],
                        quant_non_block_modules=True, device="cuda:0", save_dir=str(tmp / level), fused_forward=level)
        drv.quantize({k: T[v] for k, v in MIXED.items()})
        torch.cuda.synchronize()
        w["fused"][level] = " ".join(drv._fused_modules)
        w["verdicts"][level] = dict(forward_fused._qkn_verdict)
    w["gguf"] = str(convert(Path(hf), tmp / "exact", tmp / "m.gguf", "f16"))
    ids = TQ.tiny_calib(n=3, L=64, seed=29)
    torch.save(ids, str(tmp / "ids.pt"))
    w["ids"], w["ids_pt"] = ids, str(tmp / "ids.pt")
    return w


def test_quantize_saves_identical_bytes_with_the_kernel_on_and_off(world):
    assert "Qwen3Attention.forward" in world["fused"]["exact"] and not world["fused"]["off"]
    assert world["verdicts"]["exact"] and all(world["verdicts"]["exact"].values())  # verified on the run's own inputs, and used
    a, b = _tree_bytes(world["tmp"] / "exact"), _tree_bytes(world["tmp"] / "off")
    assert len(a) >= 7 * TQ.LAYERS + 2 and sorted(a) == sorted(b)
    for f in a:
        assert a[f] == b[f], f


def test_convert_load_ppleval_and_generate(world):
    from test_gpu_eval import run_ppleval
    from gptq_gguf_toolkit_amd import generate, gguf_loader
    from gptq_gguf_toolkit_amd.gguf_writer import read_gguf
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    kv, ts = read_gguf(world["gguf"])
    assert kv["general.architecture"] == "qwen3" and kv["tokenizer.ggml.pre"] == "qwen2"
    assert ts["blk.0.attn_q.weight"][1] == 11 and ts["blk.1.attn_k.weight"][1] == 10 and ts["blk.0.attn_q_norm.weight"][1] == 0
    dense = gguf_loader.load_into_model(_load_hf(world["hf"]), world["gguf"])
    packed = gguf_loader.load_into_model(_load_hf(world["hf"]), world["gguf"], packed=True)
    mods = [m for m in packed.modules() if isinstance(m, PackedLinear)]
    assert len(mods) == 7 * TQ.LAYERS and all(m.row_src is None for m in mods)  # no rotary row gather for "qwen3"
    live = torch.load(os.path.join(world["tmp"], "exact", "model.layers.0.self_attn.q_proj", "data.pth"), weights_only=True)
    assert live["qweight"].shape == dense.model.layers[0].self_attn.q_proj.weight.shape
    src = _load_hf(world["hf"])
    for n in ("q_norm", "k_norm"):  # the norms come back bit for bit
        assert torch.equal(getattr(dense.model.layers[1].self_attn, n).weight, getattr(src.model.layers[1].self_attn, n).weight)
    res_d, _ = run_ppleval(world, "dense", "--gguf", world["gguf"])
    res_p, _ = run_ppleval(world, "packed", "--gguf", world["gguf"], "--packed")
    nll_d = math.log(res_d["perplexity_results"][world["ids_pt"]])
    nll_p = math.log(res_p["perplexity_results"][world["ids_pt"]])
    # the rule of tests/test_gpu_packed_vocab.py::test_ppleval_packed_vocab and tests/test_gpu_moe_model.py: ln ppl is the mean of
    # lse(x) - x[label] over the rows, 2-Lipschitz in max |x|.  floor = max |dense fp16 logits - the same weights' fp32 logits| on
    # the evaluation tokens; the packed model's logits are held to 2 floor of the fp32 copy, so |ln ppl(packed) - ln ppl(fp32)|
    # <= 4 floor and |ln ppl(dense) - ln ppl(fp32)| <= 2 floor, hence the two loads differ by at most 6 floor from each other
    data = torch.cat(world["ids"]).cuda()
    with torch.no_grad():
        l_dense, l_packed = dense(data).logits.float(), packed(data).logits.float()
        ref = copy.deepcopy(dense).float()(data).logits
        nll_32 = float(torch.nn.functional.cross_entropy(ref[:, :-1].reshape(-1, TQ.VOCAB).double(), data[:, 1:].reshape(-1)))
    floor, err = float((l_dense - ref).abs().max()), float((l_packed - ref).abs().max())
    print(f"\nppleval --gguf on the tiny Qwen3: NLL dense {nll_d!r}, packed {nll_p!r}, the same weights in fp32 {nll_32!r}; "
          f"floor {floor!r}, packed logits against fp32 {err!r}")
    assert np.isfinite(nll_d) and np.isfinite(nll_p)
    assert floor > 0 and err <= 2 * floor
    assert abs(nll_p - nll_32) <= 4 * floor and abs(nll_d - nll_32) <= 2 * floor and abs(nll_p - nll_d) <= 6 * floor
    out = world["tmp"] / "gen.json"
    with redirect_stdout(io.StringIO()):
        generate.main(["--model_name_or_path", world["hf"], "--gguf", world["gguf"], "--packed", "--prompt_ids", world["ids_pt"],
                       "--max_new_tokens", "4", "--dtype", "float16", "--attn_implementation", "eager", "--output_file", str(out)])
    res = json.loads(out.read_text())
    assert len(res["prompts"]) == 3 and all(len(r["new_ids"]) == 4 and all(0 <= i < TQ.VOCAB for i in r["new_ids"]) for r in res["prompts"])


def test_level_db_equals_convert_and_split_and_stitches_verified(tmp_path):
    """quantize_levels(level_db=...) of Q3_K + Q4_K against convert() per level + gguf_splitter --gguf-layers --exact, byte for
    byte (as tests/test_gpu_level_db.py asserts for Llama: here no q / k row gather on either side), then a mixed
    configuration stitched from the database with verify=True."""
    from gptq_gguf_toolkit_amd import evo_quant_search as S
    from gptq_gguf_toolkit_amd import gguf_splitter
    from gptq_gguf_toolkit_amd.gguf_stitcher import stitch_search_result
    from gptq_gguf_toolkit_amd.gguf_writer import read_gguf
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import convert
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    from gptq_gguf_toolkit_amd.quantizer import Quantizer
    keep = os.environ.get("GQ_SAVE_SLOT_MB")
    os.environ["GQ_SAVE_SLOT_MB"] = "8"
    try:
        model = TQ.tiny_qwen3()  # fp32, as the Llama test's
        model_dir = tmp_path / "model"
        model.save_pretrained(str(model_dir))
        model = model.cuda()
        data = [([], {"input_ids": ids}) for ids in TQ.tiny_calib()]
        os.makedirs(tmp_path / "trees")
        drv = Quantizer(model, data_loader=data, quantizable_modules=TQ.LINEARS, quantizer_kwargs=QUANT_KW,
                        pre_block_modules=["model.embed_tokens"], block_modules="model.layers", post_block_modules=["lm_head"],
                        quant_non_block_modules=False, device="cuda:0", save_dir=str(tmp_path / "trees"))
        db, db2 = tmp_path / "db", tmp_path / "db2"
        drv.quantize_levels([T.Q3_K, T.Q4_K], T.Q4_K, level_db=str(db), level_db_model=str(model_dir), level_db_vocab=False)
        torch.cuda.synchronize()
        for lv in ("Q3_K", "Q4_K"):
            convert(Path(model_dir), tmp_path / "trees" / lv, tmp_path / f"{lv}.gguf", vocab=False)
            gguf_splitter.main([str(tmp_path / f"{lv}.gguf"), str(db2), "--gguf-layers", "--exact"])
    finally:
        if keep is None:
            os.environ.pop("GQ_SAVE_SLOT_MB", None)
        else:
            os.environ["GQ_SAVE_SLOT_MB"] = keep
    files = sorted(os.path.relpath(os.path.join(d, f), db2) for d, _, fs in os.walk(db2) for f in fs if f.endswith(".pth"))
    n_lin = 7 * TQ.LAYERS
    assert len(files) == n_lin * 2 + (4 * TQ.LAYERS + 1) + 2  # the Linears at two levels; the norms (q / k norms too); embed, output
    assert files == sorted(os.path.relpath(os.path.join(d, f), db) for d, _, fs in os.walk(db) for f in fs if f.endswith(".pth"))
    for f in files:
        a, b = np.fromfile(db2 / f, np.uint8), np.fromfile(db / f, np.uint8)
        assert a.size == b.size and np.array_equal(a, b), f
    ma, mb = json.load(open(db2 / "manifest.json")), json.load(open(db / "manifest.json"))
    assert ma["metadata"] == mb["metadata"] and list(ma["metadata"]) == list(mb["metadata"]) and list(ma["layers"]) == list(mb["layers"])
    names = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and "layers" in n]
    assert len(names) == n_lin
    levels = S.scan_available_bitwidths(str(db), names)
    widths = [bw for bw, _ in levels[names[0]]]
    assert len(widths) == 2
    assignment = {n: widths[(i + i // 7) % 2] for i, n in enumerate(names)}
    assignment["model.layers.0.self_attn.q_proj"], assignment["model.layers.0.self_attn.k_proj"] = widths[0], widths[1]
    cfg = tmp_path / S.configuration_name("kl", 4.0)
    cfg.write_text(S.configuration_text([names], [[assignment[n] for n in names]], levels))
    out = stitch_search_result(str(db), str(cfg), str(tmp_path / "mixed.gguf"), verify=True)
    kv, ts = read_gguf(out)
    assert kv["general.architecture"] == "qwen3" and {ts["blk.0.attn_q.weight"][1], ts["blk.0.attn_k.weight"][1]} == {11, 12}
