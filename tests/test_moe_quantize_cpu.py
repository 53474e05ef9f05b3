"""Fused-expert MoE models through the Quantizer, host side (no GPU): include/gptq_gguf_moe_calib.h declared, exported, bound
and refusing before the first HIP call; the contract of gq_fwd_moe_combine (tests/moe_combine_spec.py) against transformers'
own sequence on the CPU; moe_calibration.CalibExperts' "loop" forward against the MixtralExperts it stands in for; the driver
on a tiny transformers-5.x Mixtral with tests/fake_ops.py (the oracle) as the backend, its tree under the checkpoint's names,
the packer's stacked expert tensors; the refusals."""
import ctypes
import os
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")
sys.path.insert(0, os.path.join(ROOT, "tests"))

from moe_combine_spec import bits, combine_hf, combine_spec, route, transposed_pairs  # noqa: E402

A = 256  # any 16-byte aligned address, never dereferenced
F32, F16, BF16 = 0, 1, 2
BAD_TYPE, BAD_SHAPE, NULL = -1, -2, -6
E5, K, H, I, V, LAYERS = 5, 2, 256, 512, 512, 2
QCFG = {"q_proj": "Q6_K", "k_proj": "Q6_K", "v_proj": "Q6_K", "o_proj": "Q6_K", "w1": "Q3_K", "w2": "Q4_K", "w3": "Q3_K",
        "embed_tokens": "Q6_K", "lm_head": "Q6_K"}
QID = {"Q3_K": 11, "Q4_K": 12, "Q6_K": 14}


# ------------------------------------------------------------------------------------------------ header and binding
def test_moe_calib_header_is_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi, ops
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_moe_calib.h")).read()
    declared = set(re.findall(r"^int (gq_[a-z0-9_]+)\s*\(", hdr, re.M))
    L = _cabi.lib()
    assert declared == set(_cabi.EXPORTS_MOE_CALIB) == {"gq_fwd_moe_combine"}
    assert hasattr(ctypes.CDLL(_cabi.SO_PATH), "gq_fwd_moe_combine") and len(L.gq_fwd_moe_combine.argtypes) == 13
    assert len(_cabi.EXPORTS) == 48 and L.gq_abi_version() == _cabi.ABI_VERSION == 6  # additive: both stay
    assert '#include "gptq_gguf_moe_gemm.h"' in hdr
    k = int(re.search(r"#define GQ_MOE_COMBINE_MAX_K (\d+)", hdr).group(1))
    assert k == _cabi.MOE_COMBINE_MAX_K == ops.MOE_COMBINE_MAX_K == 8
    assert callable(ops.fwd_moe_combine)
    assert "(48 symbols)" in open(os.path.join(ROOT, "README.md")).read()
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "gq_fwd_moe_combine" in text and "gptq_gguf_moe_calib.h" in text, doc


def test_moe_combine_refusals_need_no_device():
    """Every refusal differs from a good call in one argument; host pointers do, the checks precede the first HIP call."""
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()

    def refused(status, word, y=A, pe=A, es=A, order=A, w=A, w_dtype=F32, T=4, K=2, E=3, H=16, dtype=F16, out=A):
        rc = L.gq_fwd_moe_combine(y, pe, es, order, w, w_dtype, T, K, E, H, dtype, out, None)
        msg = L.gq_last_error().decode()
        assert rc == status and word in msg and "gq_fwd_moe_combine" in msg, (rc, msg)

    refused(BAD_SHAPE, "H=12", H=12)
    refused(BAD_SHAPE, "H=0", H=0)
    refused(BAD_SHAPE, "K=0", K=0)
    refused(BAD_SHAPE, "K=9", K=9)
    for arg in ("y", "pe", "es", "order", "w", "out"):
        refused(NULL, "is NULL", **{arg: None})
    refused(BAD_SHAPE, "y not 16-byte aligned", y=A + 8)
    refused(BAD_SHAPE, "out not 16-byte aligned", out=A + 2)
    refused(BAD_SHAPE, "order not 4-byte aligned", order=A + 2)
    refused(BAD_SHAPE, "w not 4-byte aligned", w=A + 2)
    refused(BAD_SHAPE, "w not 2-byte aligned", w=A + 1, w_dtype=F16)
    refused(BAD_TYPE, "dtype 3", dtype=3)
    refused(BAD_TYPE, "dtype 0", dtype=F32)
    refused(BAD_TYPE, "w_dtype 2", w_dtype=BF16)  # neither fp32 nor y's dtype
    refused(BAD_SHAPE, "E=0", E=0)
    refused(BAD_SHAPE, f"E={_cabi.MOE_ROUTE_MAX_EXPERTS + 1}", E=_cabi.MOE_ROUTE_MAX_EXPERTS + 1)
    refused(BAD_SHAPE, "T=0", T=0)
    refused(BAD_SHAPE, f"T={_cabi.MOE_ROUTE_MAX_PAIRS // 2 + 1}", T=_cabi.MOE_ROUTE_MAX_PAIRS // 2 + 1)
    # the documented order: dtype, w_dtype, NULL, E, K, T, H, alignments
    refused(BAD_TYPE, "dtype 3", dtype=3, y=None, E=0, K=0, T=0, H=12, out=A + 2)
    refused(NULL, "y is NULL", y=None, E=0, K=0, T=0, H=12, out=A + 2)
    refused(BAD_SHAPE, "E=0", E=0, K=0, T=0, H=12, out=A + 2)
    refused(BAD_SHAPE, "K=0", K=0, T=0, H=12, out=A + 2)
    refused(BAD_SHAPE, "T=0", T=0, H=12, out=A + 2)
    refused(BAD_SHAPE, "H=12", H=12, out=A + 2)
    # the limits themselves pass: the refusal is a later check's
    refused(BAD_SHAPE, "out not 16-byte aligned", E=_cabi.MOE_ROUTE_MAX_EXPERTS, K=8, T=_cabi.MOE_ROUTE_MAX_PAIRS // 8, H=8, out=A + 4)


def test_ops_fwd_moe_combine_refusals_name_the_value():
    from gptq_gguf_toolkit_amd import _cabi, ops
    T, E = 4, 3
    y, w = torch.zeros(T * K, 16, dtype=torch.float16), torch.zeros(T, K)
    pe, rt = torch.zeros(T * K, dtype=torch.int32), (torch.zeros(E + 1, dtype=torch.int32), torch.zeros(T * K, dtype=torch.int32))
    for kw, word in ((dict(y=y.float()), "fp16 or bf16"), (dict(y=y[:, :12].contiguous()), "H=12"), (dict(w=w.double()), "fp32 or"),
                     (dict(w=torch.zeros(T, 9)), "K=9"), (dict(w=torch.zeros(3, K)), r"T=3 \* K=2 != P=8"),
                     (dict(pair_expert=pe.long()), "pair_expert must be a contiguous int32"),
                     (dict(route=(rt[0][:-1], rt[1])), r"expert_start must be a contiguous int32 \[4\]"), (dict(E=0), "E=0"),
                     (dict(), "CPU")):  # every argument good but on the host: there is no CPU path
        args = dict(y=y, pair_expert=pe, route=rt, w=w, E=E)
        args.update(kw)
        with pytest.raises(_cabi.GQError, match=word):
            ops.fwd_moe_combine(**args)


# ------------------------------------------------------------------------------------------------ the contract
def combine_case(T, Kc, E, Hc, dt, w_dt, seed=0, unused=None, masked=(), all_masked=None, twice=None, neg_zero=False):
    """(y in expert-sorted order, index [T, Kc], w [T, Kc]): distinct experts per token out of [0, E) without `unused`; `masked`
    (t, k) pairs get the id E; token `all_masked` only such ids; token `twice` names one expert in two slots; neg_zero: token 0
    keeps its first pair only, and that product is -0 in element 0."""
    g = torch.Generator().manual_seed(seed)
    pool = [e for e in range(E) if e != unused]
    idx = torch.stack([torch.tensor(pool)[torch.randperm(len(pool), generator=g)[:Kc]] for _ in range(T)]) if Kc <= len(pool) \
        else torch.stack([torch.tensor(pool)[torch.randint(0, len(pool), (Kc,), generator=g)] for _ in range(T)])
    for t, k in masked:
        idx[t, k] = E
    if all_masked is not None:
        idx[all_masked] = E
    if twice is not None and Kc > 1:
        idx[twice, 1] = idx[twice, 0]
    if neg_zero:
        idx[0, 1:] = E  # token 0 keeps one pair: its only product is the -0
    w = torch.softmax(torch.randn(T, Kc, generator=g), -1).to(w_dt)
    y = (torch.randn(T * Kc, Hc, generator=g) * 3).to(dt)
    if neg_zero:
        y[route(transposed_pairs(idx), E)[1].index(0), 0] = -0.0  # pair (t = 0, k = 0); w > 0
    return y, idx, w


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_combine_spec_is_transformers_sequence_on_the_cpu(dt):
    """The loop restatement against zeros + index_add_ per expert, where no token names an expert twice: bit for bit, a masked
    pair, a token without experts and a -0 first product included."""
    for w_dt in (torch.float32, dt):
        y, idx, w = combine_case(7, 2, 5, 264, dt, w_dt, unused=4, masked=[(3, 1)], all_masked=5, neg_zero=True)
        got = combine_spec(y, idx, w, 5)
        assert torch.equal(bits(got), bits(combine_hf(y, idx, w, 5)))
        assert bool((got[5] == 0).all()) and int(bits(got)[0, 0]) == 0  # +0, not -0
    y, idx, w = combine_case(7, 2, 5, 8, dt, torch.float32, twice=2)  # the tie rule: k ascending
    t, e = 2, int(idx[2, 0])
    _, order = route(transposed_pairs(idx), 5)
    v = [(y[order.index(k * 7 + t)].float() * w[t, k]).to(dt) for k in (0, 1)]
    assert int(idx[t, 1]) == e and torch.equal(combine_spec(y, idx, w, 5)[t], ((0 + v[0].float()).to(dt).float() + v[1].float()).to(dt))


# ------------------------------------------------------------------------------------------------ "loop" against the module
def test_loop_forward_is_the_original_module_and_feeds_the_hooks():
    import moe_gguf
    from transformers.models.mixtral.modeling_mixtral import MixtralSparseMoeBlock
    from gptq_gguf_toolkit_amd import moe_calibration as mc
    torch.manual_seed(0)
    holder = torch.nn.Module()
    holder.mlp = MixtralSparseMoeBlock(moe_gguf.config()).float().eval()
    orig = holder.mlp.experts
    with torch.no_grad():
        for p in orig.parameters():
            p.copy_(torch.randn(p.shape) * 0.05)
    T, E = 96, moe_gguf.E
    g = torch.Generator().manual_seed(1)
    x = torch.randn(T, moe_gguf.H, generator=g)
    idx = torch.stack([torch.randperm(3, generator=g)[:2] for _ in range(T)])  # never names expert 3
    w = torch.softmax(torch.randn(T, 2, generator=g), -1)
    with torch.no_grad():
        want = orig(x, idx, w)
    installed = mc.install(holder, "mlp.", r"experts\.\d+\.w[123]$")
    stand_in = holder.mlp.experts
    assert isinstance(stand_in, mc.CalibExperts) and stand_in.mode == "loop" and len(installed) == 1
    names = [n for n, m in holder.named_modules() if isinstance(m, torch.nn.Linear)]
    assert names == [f"mlp.experts.{e}.{r}" for e in range(E) for r in ("w1", "w3", "w2")]
    seen = []
    for n, m in holder.named_modules():
        if isinstance(m, torch.nn.Linear):
            e, r = n.split(".")[-2:]
            src = orig.gate_up_proj if r != "w2" else orig.down_proj
            view = {"w1": src[int(e), :moe_gguf.I], "w3": src[int(e), moe_gguf.I:], "w2": src[int(e)]}[r]
            assert m.weight.data_ptr() == view.data_ptr() and m.weight.shape == view.shape and torch.equal(m.weight, view)  # a view
            m.register_forward_pre_hook(lambda mod, inp, n=n: seen.append((n, inp[0])))
    with torch.no_grad():
        got = stand_in(x, idx, w)
    assert torch.equal(got, want)
    assert [n for n, _ in seen] == [f"mlp.experts.{e}.{r}" for e in range(3) for r in ("w1", "w3", "w2")]  # expert 3: never called
    act = orig.act_fn
    for e in range(3):
        top_k_pos, token_idx = torch.where((idx == e).T)  # transformers' order: by choice, then by token
        cur = x[token_idx]
        gate, up = torch.nn.functional.linear(cur, orig.gate_up_proj[e]).chunk(2, dim=-1)
        (_, x1), (_, x3), (_, x2) = seen[3 * e:3 * e + 3]
        assert x1 is x3 and torch.equal(x1, cur) and torch.equal(x2, act(gate) * up)
    # a write-back through a child lands in the fused parameter
    stand_in.expert(1).w3.weight.data = torch.full((moe_gguf.I, moe_gguf.H), 2.0)
    assert bool((orig.gate_up_proj[1, moe_gguf.I:] == 2).all()) and not bool((orig.gate_up_proj[1, :moe_gguf.I] == 2).any())
    mc.restore(installed)
    assert holder.mlp.experts is orig and installed == []


def test_names_of_the_trees_are_the_checkpoints():
    from gptq_gguf_toolkit_amd import moe_calibration as mc
    assert mc.NAME_TABLE == ((".mlp.experts.", ".block_sparse_moe.experts."),)
    assert mc.checkpoint_name("model.layers.3.mlp.experts.7.w2") == "model.layers.3.block_sparse_moe.experts.7.w2"
    for same in ("model.layers.3.self_attn.q_proj", "model.layers.0.mlp.gate", "model.layers.0.mlp.experts.gate_up_proj",
                 "model.layers.0.block_sparse_moe.experts.1.w1", "lm_head"):
        assert mc.checkpoint_name(same) == same
    assert mc.synthesized_names("a.experts", 2) == ["a.experts.0.w1", "a.experts.0.w3", "a.experts.0.w2", "a.experts.1.w1",
                                                    "a.experts.1.w3", "a.experts.1.w2"]
    from tiny_moe import MOE_REGEX
    assert all(re.search(MOE_REGEX, n) for n in mc.synthesized_names("model.layers.0.mlp.experts", 2))


# ------------------------------------------------------------------------------------------------ the driver
def tiny_mixtral(hidden_act="silu"):
    """A 2-layer fp32 MixtralForCausalLM with E = 5 whose last router row is made to lose: every embedding carries a large
    positive component along dimension 0 (it dominates the residual stream and survives the RMSNorm), the last expert's
    router row is strongly negative there."""
    from transformers import MixtralConfig, MixtralForCausalLM
    torch.manual_seed(0)
    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_hidden_layers=LAYERS, num_attention_heads=4, num_key_value_heads=2,
                        num_local_experts=E5, num_experts_per_tok=K, vocab_size=V, max_position_embeddings=128,
                        tie_word_embeddings=False, router_jitter_noise=0.0, hidden_act=hidden_act)
    model = MixtralForCausalLM(cfg).float().eval()
    with torch.no_grad():
        model.model.embed_tokens.weight[:, 0] += 6.0
        for layer in model.model.layers:
            layer.mlp.gate.weight[E5 - 1] = 0.0
            layer.mlp.gate.weight[E5 - 1, 0] = -4.0
    return model


def calib(n=6, L=64, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, V, (1, L), generator=g) for _ in range(n)]


def make_quantizer(model, save_dir, regex=None, device="cpu", **kw):
    from tiny_moe import MOE_REGEX
    from gptq_gguf_toolkit_amd.quantizer import Quantizer
    data = [([], {"input_ids": ids}) for ids in calib()]
    return Quantizer(model, data_loader=data, quantizable_modules=regex or MOE_REGEX,
                     quantizer_kwargs=dict(rel_damp=0.01, block_size=128, act_order=False, quant_scale="absmax",
                                           static_groups=False, rmin=-1.0, rdelta=0.1, nstep=20, verbose=False),
                     pre_block_modules=["model.embed_tokens"], block_modules="model.layers", post_block_modules=["lm_head"],
                     quant_non_block_modules=True, device=device, save_dir=str(save_dir), **kw)


def qconfig():
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    return {k: T[v] for k, v in QCFG.items()}


def tree_names():
    want = ["lm_head", "model.embed_tokens"]
    for i in range(LAYERS):
        want += [f"model.layers.{i}.self_attn.{p}_proj" for p in "qkvo"]
        want += [f"model.layers.{i}.block_sparse_moe.experts.{e}.w{k}" for e in range(E5) for k in (1, 2, 3)]
    return sorted(want)


def load_tree(save_dir, name):
    d = torch.load(os.path.join(save_dir, name, "data.pth"), weights_only=True)
    return d, [d["qweight"], d["super_group_scale"], d["group_scale_quant"], d["super_group_zero"], d["group_zero_quant"]]


@pytest.fixture(scope="module")
def driven(tmp_path_factory):
    """(model after the run, its fused weights before it, hf dir, save dir): ONE Quantizer.quantize with the oracle backend."""
    import fake_ops
    fake_ops.install()
    tmp = tmp_path_factory.mktemp("moe_quant")
    model = tiny_mixtral()
    hf, save = tmp / "hf", tmp / "tree"
    model.save_pretrained(str(hf), safe_serialization=True)
    before = {n: p.detach().clone() for n, p in model.named_parameters() if ".experts." in n}
    experts = [layer.mlp.experts for layer in model.model.layers]
    os.makedirs(save)
    make_quantizer(model, save).quantize(qconfig())
    assert all(layer.mlp.experts is m for layer, m in zip(model.model.layers, experts))  # restored, by identity
    return model, before, hf, str(save)


def test_driver_writes_every_expert_tree_under_the_checkpoints_names(driven):
    """Fails on a Quantizer that only sees nn.Linear modules: no expert tree is written there."""
    import fake_ops
    model, before, _, save = driven
    assert sorted(os.listdir(save)) == tree_names()
    for i in range(LAYERS):
        ex = model.model.layers[i].mlp.experts
        assert type(ex).__name__ == "MixtralExperts"
        for e in range(E5):
            for r, rows in (("w1", slice(0, I)), ("w3", slice(I, 2 * I)), ("w2", None)):
                d, five = load_tree(save, f"model.layers.{i}.block_sparse_moe.experts.{e}.{r}")
                assert d["q_type"] == QID[QCFG[r]] and tuple(d["qweight"].shape) == ((H, I) if r == "w2" else (I, H))
                have = ex.down_proj[e] if r == "w2" else ex.gate_up_proj[e, rows]
                assert torch.equal(have.detach(), fake_ops.dequantize(d["q_type"], *five, out_dtype=torch.float32)), (i, e, r)
                key = f"model.layers.{i}.mlp.experts." + ("down_proj" if r == "w2" else "gate_up_proj")
                w0 = before[key][e] if r == "w2" else before[key][e, rows]
                assert not torch.equal(have.detach(), w0)
                if e == E5 - 1:  # never routed to: H = I, round-to-nearest of its weights, bit for bit
                    rtn = fake_ops.rtn_quantize(w0.contiguous(), d["q_type"])
                    assert all(torch.equal(a, b) for a, b in zip(five, rtn)), (i, r)
        for p in "qkvo":
            assert load_tree(save, f"model.layers.{i}.self_attn.{p}_proj")[0]["q_type"] == 14


def test_packer_stacks_the_quantized_experts(driven, tmp_path, monkeypatch):
    """Fails on a tree without expert entries: the experts then come out F16."""
    import fake_ops
    from gptq_gguf_toolkit_amd import packing_utils
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import convert
    monkeypatch.setattr(packing_utils, "_ops", fake_ops)  # no GPU here: the oracle's bit-packer stands in
    monkeypatch.setattr(packing_utils, "_dev", lambda t: t.contiguous())
    _, _, hf, save = driven
    out = convert(Path(hf), Path(save), tmp_path / "m.gguf", "f16", vocab=False)
    tensors = read_tensors(str(out))
    for i in range(LAYERS):
        for role, r, (R, C) in (("gate", "w1", (I, H)), ("up", "w3", (I, H)), ("down", "w2", (H, I))):
            dims, gt, raw = tensors[f"blk.{i}.ffn_{role}_exps.weight"]
            assert gt == QID[QCFG[r]] and tuple(dims) == (C, R, E5)
            per = len(raw) // E5
            for e in range(E5):
                d, five = load_tree(save, f"model.layers.{i}.block_sparse_moe.experts.{e}.{r}")
                want = packing_utils.pack_tensor(d["q_type"], *five)
                assert bytes(raw[e * per:(e + 1) * per]) == want.tobytes(), (i, role, e)


def read_tensors(path):
    """{name: (ggml dims innermost first, ggml type, payload bytes)} from the GGUF v3 specification: after the key/value data
    (skipped with tests/gguf_spec_reader.py's grammar) come n_tensors x {string name, u32 n_dims, u64 dims[n_dims], u32 type,
    u64 offset}; the data section starts at the next multiple of 32 and the offsets are relative to it."""
    import struct
    from gguf_spec_reader import read_kv
    sizes = {0: (1, 4), 1: (1, 2), 10: (256, 84), 11: (256, 110), 12: (256, 144), 13: (256, 176), 14: (256, 210)}  # ggml-common.h
    scalar = {0: 1, 1: 1, 2: 2, 3: 2, 4: 4, 5: 4, 6: 4, 7: 1, 10: 8, 11: 8, 12: 8}
    buf = open(path, "rb").read()
    kv, _, n_tensors = read_kv(path)
    pos = 24

    def skip(t):
        nonlocal pos
        if t == 8:
            pos += 8 + struct.unpack_from("<Q", buf, pos)[0]
        elif t == 9:
            et, cnt = struct.unpack_from("<IQ", buf, pos)
            pos += 12
            for _ in range(cnt):
                skip(et)
        else:
            pos += scalar[t]

    for _ in range(len(kv)):
        skip(8)
        t = struct.unpack_from("<I", buf, pos)[0]
        pos += 4
        skip(t)
    infos = []
    for _ in range(n_tensors):
        n = struct.unpack_from("<Q", buf, pos)[0]
        name = buf[pos + 8:pos + 8 + n].decode("utf-8")
        pos += 8 + n
        nd = struct.unpack_from("<I", buf, pos)[0]
        dims = struct.unpack_from(f"<{nd}Q", buf, pos + 4)
        gt, off = struct.unpack_from("<IQ", buf, pos + 4 + 8 * nd)
        pos += 4 + 8 * nd + 12
        infos.append((name, tuple(dims), gt, off))
    data0 = (pos + 31) // 32 * 32
    out = {}
    for name, dims, gt, off in infos:
        bs, ts = sizes[gt]
        nbytes = int(np.prod(dims)) // bs * ts
        assert off % 32 == 0 and data0 + off + nbytes <= len(buf), name
        out[name] = (dims, gt, buf[data0 + off:data0 + off + nbytes])
    return out


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_module(tmp_path):
    import fake_ops
    from tiny_moe import MOE_REGEX
    from gptq_gguf_toolkit_amd import moe_calibration as mc
    fake_ops.install()
    model = tiny_mixtral(hidden_act="gelu")
    experts = model.model.layers[0].mlp.experts
    with pytest.raises(NotImplementedError, match=r"model\.layers\.0\.mlp\.experts.*activation"):
        make_quantizer(model, tmp_path).quantize(qconfig())
    assert model.model.layers[0].mlp.experts is experts
    model = tiny_mixtral()
    with pytest.raises(NotImplementedError, match=r"quantize_levels: model\.layers\.0\.mlp\.experts"):
        make_quantizer(model, tmp_path).quantize_levels([12], 12)
    # an unknown layout: fused along dim 0, but not gate_up_proj [E, 2I, H] / down_proj [E, H, I]
    odd = torch.nn.Module()
    odd.layers = torch.nn.ModuleList([torch.nn.Module()])
    odd.layers[0].mlp = torch.nn.Module()
    odd.layers[0].mlp.experts = torch.nn.Module()
    odd.layers[0].mlp.experts.w13 = torch.nn.Parameter(torch.zeros(3, 8, 4))
    with pytest.raises(NotImplementedError, match=r"layers\.0\.mlp\.experts.*gate_up_proj"):
        mc.install(odd, "layers.0.", MOE_REGEX)
    assert mc.install(odd, "layers.0.", r"(q|k|v|o)_proj$") == []  # a regex that names no expert: nothing is touched


def test_a_regex_without_experts_runs_as_before(tmp_path):
    import fake_ops
    fake_ops.install()
    model = tiny_mixtral()
    before = {n: p.detach().clone() for n, p in model.named_parameters() if ".experts." in n}
    make_quantizer(model, tmp_path, regex=r".*layers.*(q|k|v|o)_proj$").quantize(qconfig())
    want = ["lm_head", "model.embed_tokens"] + [f"model.layers.{i}.self_attn.{p}_proj" for i in range(LAYERS) for p in "qkvo"]
    assert sorted(os.listdir(tmp_path)) == sorted(want)
    assert all(torch.equal(p.detach(), before[n]) for n, p in model.named_parameters() if n in before)
