"""A MoE .gguf through the loader, PackedExperts, ppleval and generate on the GPU: the 2-layer Mixtral of tests/moe_gguf.py
(4 experts, top-2; the six packed types spread over the expert tensors of the two layers) loaded dense and packed."""
import copy
import io
import json
import math
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

import moe_gguf
from conftest import ROOT
from test_gpu_eval import run_ppleval
from test_gpu_packed_vocab import N_PROMPT, incremental

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

ID_SEED = 29  # tiny_calib(n=3, L=64, seed=29): the dense and the packed load route every token of these ids alike (test below)
E, K, H, I = moe_gguf.E, moe_gguf.K, moe_gguf.H, moe_gguf.I
ROLE_FILE = {"gate": "ffn_gate_exps", "up": "ffn_up_exps", "down": "ffn_down_exps"}


def i16(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from make_golden_shim import tiny_calib
    from gptq_gguf_toolkit_amd import gguf_loader
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    tmp = tmp_path_factory.mktemp("moe")
    hf, gguf = tmp / "hf", tmp / "moe.gguf"
    moe_gguf.build_hf(hf)
    types = moe_gguf.write_gguf(moe_gguf.load_hf(hf), gguf)
    ids = tiny_calib(n=3, L=64, seed=ID_SEED)
    torch.save(ids, str(tmp / "ids.pt"))
    dense = gguf_loader.load_into_model(moe_gguf.load_hf(hf), str(gguf))
    packed = gguf_loader.load_into_model(moe_gguf.load_hf(hf), str(gguf), packed=True)
    fp32 = copy.deepcopy(dense).float()
    return dict(tmp=tmp, hf=str(hf), gguf=str(gguf), types=types, ids=ids, ids_pt=str(tmp / "ids.pt"), dense=dense,
                packed=packed, fp32=fp32)


def file_decode(world, name):
    """dequantize_blocks of the file's bytes of one merged tensor -> fp16 [E, R, C]."""
    from gptq_gguf_toolkit_amd import ops
    from gptq_gguf_toolkit_amd.gguf_writer import parse_gguf
    _, tensors, buf = parse_gguf(world["gguf"], mmap=True)
    (shape, gt, off, n), = [(s, g, o, n) for nm, s, g, o, n in tensors if nm == name]
    raw = torch.from_numpy(np.array(buf[off:off + n])).cuda()
    return ops.dequantize_blocks(gt, raw.view(shape[0] * shape[1], -1), torch.float16).view(*shape), raw, gt


# ------------------------------------------------------------------------------------------------ the two loads
def test_dense_load_is_the_decode_of_the_files_bytes(world):
    for n in range(moe_gguf.LAYERS):
        ex = world["dense"].model.layers[n].mlp.experts
        assert type(ex).__name__ == "MixtralExperts" and ex.gate_up_proj.shape == (E, 2 * I, H)
        for role, got in (("gate", ex.gate_up_proj[:, :I]), ("up", ex.gate_up_proj[:, I:]), ("down", ex.down_proj)):
            want, _, gt = file_decode(world, f"blk.{n}.{ROLE_FILE[role]}.weight")
            assert gt == moe_gguf.EXPERT_TYPES[n][role] and torch.equal(i16(got.data), i16(want)), (n, role)
        router = world["dense"].model.layers[n].mlp.gate.weight
        assert router.shape == (E, H) and bool(torch.isfinite(router).all())


def test_packed_load_keeps_the_experts_as_block_bytes(world):
    from gptq_gguf_toolkit_amd import gguf_loader
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    packed, dense = world["packed"], world["dense"]
    keep = gguf_loader.packed_expert_tensors(moe_gguf.load_hf(world["hf"]), world["gguf"])
    assert keep == {f"model.layers.{n}.mlp.experts": {r: (f"blk.{n}.{ROLE_FILE[r]}.weight", moe_gguf.EXPERT_TYPES[n][r], None)
                                                      for r in ROLE_FILE} for n in range(moe_gguf.LAYERS)}
    for t in list(packed.parameters()) + list(packed.buffers()):
        assert t.dim() < 3, f"a dense {tuple(t.shape)} tensor of the packed model lives on {t.device}"
    assert not any("experts" in k for k in packed.state_dict())
    assert sum(isinstance(m, PackedLinear) for m in packed.modules()) == 4 * moe_gguf.LAYERS  # the attention Linears, as before
    assert type(packed.lm_head) is torch.nn.Linear and type(packed.model.embed_tokens) is torch.nn.Embedding
    for n in range(moe_gguf.LAYERS):
        ex, ref = packed.model.layers[n].mlp.experts, dense.model.layers[n].mlp.experts
        assert type(ex) is PackedExperts and ex.gate_up_proj.is_meta and ex.down_proj.is_meta
        assert (ex.num_experts, ex.hidden_dim, ex.intermediate_dim) == (E, H, I)
        for role in ROLE_FILE:
            blocks, q = ex.levels[role]
            _, raw, gt = file_decode(world, f"blk.{n}.{ROLE_FILE[role]}.weight")
            assert q == gt == moe_gguf.EXPERT_TYPES[n][role] and blocks.is_cuda and torch.equal(blocks.view(-1), raw)  # the bytes, once
        assert torch.equal(i16(ex.dense_gate_up()), i16(ref.gate_up_proj.data))
        assert torch.equal(i16(ex.dense_weight("down")), i16(ref.down_proj.data))
        assert type(packed.model.layers[n].mlp.gate).__name__ == "MixtralTopKRouter"
        assert torch.equal(packed.model.layers[n].mlp.gate.weight, dense.model.layers[n].mlp.gate.weight)


# ------------------------------------------------------------------------------------------------ the expert module alone
def routing(T, seed):
    g = torch.Generator().manual_seed(seed)
    w, idx = torch.topk(torch.softmax(torch.randn(T, E, generator=g), -1), K, -1)  # distinct experts per token
    return idx.cuda(), (w / w.sum(-1, keepdim=True)).cuda()


def composed(ex, x, idx, w):
    """The decode path spelled out: per pair ops.gemv_packed on the expert's slices, fwd_silu_mul, then the fp32 sum over k."""
    from gptq_gguf_toolkit_amd import ops
    sl = {r: (ex.levels[r][0].view(E, -1), ex.levels[r][1]) for r in ROLE_FILE}
    rows = []
    for t in range(x.shape[0]):
        acc = None
        for k in range(K):
            e = int(idx[t, k])
            a = ops.fwd_silu_mul(ops.gemv_packed(sl["gate"][1], sl["gate"][0][e], x[t:t + 1]),
                                 ops.gemv_packed(sl["up"][1], sl["up"][0][e], x[t:t + 1]))
            term = ops.gemv_packed(sl["down"][1], sl["down"][0][e], a).float() * w[t, k].float()
            acc = term if acc is None else acc + term
        rows.append(acc)
    return torch.cat(rows).to(x.dtype)


def fp64_and_bound(ex, x, idx, w):
    """out64 and B with |out - out64| <= B for either implementation, composed from the one-Linear bound of
    test_gpu_qgemm.py (b(y) = u |y64| + C 2^-23 (|x| |W|^T) + 2^-25, u = 2^-11: final rounding + fp32 accumulation of C
    terms in any order), all in fp64 on the decoded fp16 weights both models share:
      gate, up:  |g^ - g| <= b_g, |u^ - u| <= b_u                                   (one Linear each, C = H)
      a = silu(g) u:  silu is 1.1-Lipschitz, so |silu(g^) u^ - a| <= 1.1 b_g (|u| + b_u) + |silu(g)| b_u =: p; the product
                 is rounded to fp16 once (the fused kernel) or silu and the product once each (torch): <= 2u (|a| + p)
                 more, plus 2^-20 |a| for the device exp -> b_a
      down:      |d^ - d| <= (b_a |Wd|^T) + u (|d| + b_a |Wd|^T) + I 2^-23 ((|a| + b_a) |Wd|^T) + 2^-25 =: b_d
      sum:       sum_k w_k d_k; the decode path adds in fp32 and rounds once, the loop path and transformers round every
                 w_k d_k to fp16 and add in fp16: <= 3u sum_k (|w_k d_k| + w_k b_d,k) covers both
    B = sum_k w_k b_d,k + 3u sum_k (|w_k d_k| + w_k b_d,k).  Derived, not measured."""
    u = 2.0 ** -11
    Wg, Wu, Wd = (ex.dense_weight(r).double() for r in ("gate", "up", "down"))
    xd = x.double()
    out = torch.zeros(x.shape[0], H, dtype=torch.float64, device="cuda")
    B = torch.zeros_like(out)
    mag = torch.zeros_like(out)
    for t in range(x.shape[0]):
        for k in range(K):
            e, wk = int(idx[t, k]), float(w[t, k])
            g, up = Wg[e] @ xd[t], Wu[e] @ xd[t]
            b_g = u * g.abs() + H * 2.0 ** -23 * (Wg[e].abs() @ xd[t].abs()) + 2.0 ** -25
            b_u = u * up.abs() + H * 2.0 ** -23 * (Wu[e].abs() @ xd[t].abs()) + 2.0 ** -25
            s = torch.nn.functional.silu(g)
            a = s * up
            p = 1.1 * b_g * (up.abs() + b_u) + s.abs() * b_u
            b_a = p + 2 * u * (a.abs() + p) + 2.0 ** -20 * a.abs()
            d = Wd[e] @ a
            carried = Wd[e].abs() @ b_a
            b_d = carried + u * (d.abs() + carried) + I * 2.0 ** -23 * (Wd[e].abs() @ (a.abs() + b_a)) + 2.0 ** -25
            out[t] += wk * d
            B[t] += wk * b_d
            mag[t] += wk * (d.abs() + b_d)
    return out, B + 3 * u * mag


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("T", [1, 5, 16, 40])
def test_expert_module_alone(world, layer, T):
    """T = 1, 5, 16: the decode path, bit for bit the composition of ops.gemv_packed calls; T = 40: the loop path, with the
    GEMV (experts with at most 16 tokens) and the tile kernel (more).  Both within B of fp64, as is transformers' module on the
    dense load, so within 2 B of each other."""
    ex, ref = world["packed"].model.layers[layer].mlp.experts, world["dense"].model.layers[layer].mlp.experts
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(10 * T + layer)).half().cuda()
    idx, w = routing(T, seed=T)
    with torch.no_grad():
        got, want = ex(x, idx, w), ref(x, idx, w)
    out64, B = fp64_and_bound(ex, x, idx, w)
    assert got.shape == (T, H) and got.dtype == torch.float16 and bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    assert ex.takes_decode_path(T, K) == (T <= 16)
    if T <= 16:
        assert torch.equal(i16(got), i16(composed(ex, x, idx, w)))
    else:
        counts = torch.bincount(idx.reshape(-1).cpu(), minlength=E).tolist()
        assert min(c for c in counts if c) <= 16 < max(counts), counts  # both kernels of the loop path
    e_p, e_d = (got.double() - out64).abs(), (want.double() - out64).abs()
    print(f"layer {layer} T={T}: packed err / B = {float((e_p / B).max()):.3f}, dense err / B = {float((e_d / B).max()):.3f}, "
          f"max |packed - dense| / 2B = {float(((got.double() - want.double()).abs() / (2 * B)).max()):.3f}")
    assert bool((e_p <= B).all())
    assert bool(((got.double() - want.double()).abs() <= 2 * B).all())
    if T <= 16:  # the loop path of the same module on the same inputs: the other summation order, the same bound
        ex.grouped_max_pairs = 0
        try:
            with torch.no_grad():
                loop = ex(x, idx, w)
        finally:
            del ex.grouped_max_pairs
        assert bool(((loop.double() - out64).abs() <= B).all())


# ------------------------------------------------------------------------------------------------ the whole model
def routed(model, data):
    """The router's indices of every MoE layer for `data` [B, L], and the logits."""
    seen, hooks = [], []
    for layer in model.model.layers:
        hooks.append(layer.mlp.gate.register_forward_hook(lambda m, a, out: seen.append(out[2].clone())))
    try:
        with torch.no_grad():
            logits = model(data).logits
    finally:
        for h in hooks:
            h.remove()
    return seen, logits


def test_whole_model_routes_alike_and_scores_within_the_noise(world):
    """Precondition (inputs, not numerics): with the ids of seed ID_SEED = 29 the dense and the packed load pick the same
    experts for every token of both layers -- a flipped expert would be another model, not a rounding.
    Then the rule of test_gpu_packed_vocab.py: ln ppl is 2-Lipschitz in max |logit difference|; the packed model's logits are
    held to 2 floor of the fp32 copy of the dense load, floor = max |dense fp16 - fp32| on the same 3 x 64 tokens, so
    |ln ppl(packed) - ln ppl(fp32)| <= 4 floor."""
    data = torch.cat(world["ids"]).cuda()
    r_dense, l_dense = routed(world["dense"], data)
    r_packed, l_packed = routed(world["packed"], data)
    assert len(r_dense) == len(r_packed) == moe_gguf.LAYERS and r_dense[0].shape == (3 * 64, K)
    flips = [int((a != b).any(-1).sum()) for a, b in zip(r_dense, r_packed)]
    print(f"router decisions that differ between the dense and the packed load, per layer: {flips} of {3 * 64}")
    assert flips == [0] * moe_gguf.LAYERS, f"ids of seed {ID_SEED}: {flips} tokens routed differently"
    with torch.no_grad():
        ref = world["fp32"](data).logits
        nll = torch.nn.functional.cross_entropy(ref[:, :-1].reshape(-1, moe_gguf.V).double(), data[:, 1:].reshape(-1))
    floor = float((l_dense.float() - ref).abs().max())
    err = float((l_packed.float() - ref).abs().max())
    res, scored = run_ppleval(world, "moe_packed", "--gguf", world["gguf"], "--packed")
    from gptq_gguf_toolkit_amd import metrics
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts
    assert type(scored.model.layers[0].mlp.experts) is PackedExperts
    ppl = res["perplexity_results"][world["ids_pt"]]
    print(f"ppleval --gguf --packed: {ppl!r}; fp32 model {math.exp(float(nll))!r}; floor {floor!r}; packed logits against fp32 {err!r}")
    assert floor > 0 and err <= 2 * floor
    assert np.isfinite(ppl) and abs(math.log(ppl) - float(nll)) <= 4 * floor
    rows = metrics.nll_rows(scored, world["ids"])  # the command line reproduces the API's number
    assert abs(ppl / math.exp(float(rows.double().mean())) - 1) < 1e-12


def test_teacher_forced_steps_agree_with_the_prefill(world):
    """test_gpu_generate.py's criterion: max |packed incremental - fp32 full forward| <= 2 floor over the 16 x V logits of
    the T = 1 steps on the KV cache, floor = max |dense fp16 incremental - fp32 full forward| (torch's own 16-bit noise on
    this model).  The steps take the decode path, the prefill the loop path."""
    ids = world["ids"][0].cuda()
    with torch.no_grad():
        ref = world["fp32"](ids).logits[:, N_PROMPT:]
    floor = float((incremental(world["dense"], ids) - ref).abs().max())
    got = incremental(world["packed"], ids)
    err = float((got - ref).abs().max())
    print(f"teacher-forced decode, 16 x 512 logits: floor {floor!r}, packed against fp32 {err!r}")
    assert floor > 0 and bool(torch.isfinite(got).all())
    assert err <= 2 * floor


# ------------------------------------------------------------------------------------------------ no host synchronisation
def test_decode_step_launches_three_grouped_gemvs_per_layer(world, monkeypatch):
    from gptq_gguf_toolkit_amd import ops
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts
    calls = {"grouped": 0, "gemv_in_experts": 0, "gemv": 0, "inside": False}
    real_g, real_v, real_f = ops.gemv_packed_experts, ops.gemv_packed, PackedExperts.forward

    def grouped(*a, **k):
        calls["grouped"] += 1
        return real_g(*a, **k)

    def gemv(*a, **k):
        calls["gemv_in_experts" if calls["inside"] else "gemv"] += 1
        return real_v(*a, **k)

    def forward(self, *a, **k):
        calls["inside"] = True
        try:
            return real_f(self, *a, **k)
        finally:
            calls["inside"] = False

    monkeypatch.setattr(ops, "gemv_packed_experts", grouped)
    monkeypatch.setattr(ops, "gemv_packed", gemv)
    monkeypatch.setattr(PackedExperts, "forward", forward)
    ids = world["ids"][1].cuda()
    with torch.no_grad():
        out = world["packed"](input_ids=ids[:, :N_PROMPT], use_cache=True)
        assert calls["grouped"] == 0  # the prefill: 48 tokens, the loop path
        before = dict(calls)
        steps = 3
        for i in range(N_PROMPT, N_PROMPT + steps):
            out = world["packed"](input_ids=ids[:, i:i + 1], past_key_values=out.past_key_values, use_cache=True)
    assert calls["grouped"] == 3 * moe_gguf.LAYERS * steps
    assert calls["gemv_in_experts"] == before["gemv_in_experts"]      # none from the experts in a decode step
    assert calls["gemv"] - before["gemv"] == 4 * moe_gguf.LAYERS * steps  # the attention Linears, as before


def test_decode_path_makes_no_host_synchronisation(world):
    ex = world["packed"].model.layers[0].mlp.experts
    x = torch.randn(1, H, generator=torch.Generator().manual_seed(1)).half().cuda()
    idx, w = routing(1, seed=1)
    with torch.no_grad():
        want = ex(x, idx, w)
    probe = torch.ones(4, device="cuda")
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.nonzero()
            control = False
        except RuntimeError:
            control = True
        if control:
            with torch.no_grad():
                got = ex(x, idx, w)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    if not control:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .nonzero() raise on this build")
    assert torch.equal(i16(got), i16(want))


# ------------------------------------------------------------------------------------------------ the command lines
def test_generate_runs_on_the_packed_moe_and_its_command_line_reproduces_greedy(world):
    from gptq_gguf_toolkit_amd import generate, ppleval
    out = world["tmp"] / "gen.json"
    argv = ["--model_name_or_path", world["hf"], "--gguf", world["gguf"], "--packed", "--prompt_ids", world["ids_pt"],
            "--max_new_tokens", "4", "--dtype", "float16", "--attn_implementation", "eager", "--output_file", str(out)]
    with redirect_stdout(io.StringIO()):
        generate.main(argv)
    res = json.loads(out.read_text())
    assert res["gguf"] == world["gguf"] and res["packed"] is True and len(res["prompts"]) == 3
    args = generate.parse_args(argv)
    model = ppleval.apply_weights(ppleval.load_hf_model(args, torch.device("cuda")), args)
    for rec, ids in zip(res["prompts"], world["ids"]):
        assert rec["prompt_tokens"] == 64 and len(rec["new_ids"]) == 4 and all(0 <= i < moe_gguf.V for i in rec["new_ids"])
        assert rec["new_ids"] == generate.greedy(model, ids.cuda(), 4)[0, 64:].tolist()
    g = torch.Generator(device="cuda").manual_seed(3)
    sampled = generate.sample(world["packed"], world["ids"][0].cuda(), 4, temperature=1.5, top_k=20, generator=g)
    assert sampled.shape == (1, 68) and bool(((sampled >= 0) & (sampled < moe_gguf.V)).all())
    again = generate.sample(world["packed"], world["ids"][0].cuda(), 4, temperature=1.5, top_k=20,
                            generator=torch.Generator(device="cuda").manual_seed(3))
    assert torch.equal(sampled, again)


# ------------------------------------------------------------------------------------------------ the per-expert layout
def test_per_expert_layout_packs_each_linear_on_a_slice(tmp_path):
    """The layout of transformers up to 4.56 (`block_sparse_moe.experts.<e>.w1 / w2 / w3` are nn.Linear): with packed=True
    every such Linear becomes a PackedLinear on the e-th slice of ONE device copy of its merged tensor.  Q3_K and Q8_0 among
    the types: their slices are 2-byte aligned only.  The forward is held to test_gpu_qgemm.py's one-Linear bound."""
    import torch.nn as nn
    from gptq_gguf_toolkit_amd import gguf_loader, ops
    from gptq_gguf_toolkit_amd.gguf_writer import GGUFWriter
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    n_exp, types = 3, {"w1": ("gate", 12), "w2": ("down", 11), "w3": ("up", 8)}
    g = torch.Generator().manual_seed(4)
    w = GGUFWriter(str(tmp_path / "per.gguf"), "llama")
    w.add_tensor("blk.0.ffn_gate_inp.weight", torch.randn(n_exp, H, generator=g).numpy())
    for wname, (role, t) in types.items():
        R, C = (H, I) if role == "down" else (I, H)
        w.add_tensor(f"blk.0.ffn_{role}_exps.weight", moe_gguf._blocks(ops, (torch.randn(n_exp, R, C, generator=g) * 0.02).cuda(), t),
                     raw_dtype=t)
    w.add_tensor("output_norm.weight", torch.randn(H, generator=g).numpy())
    w.write()

    class Expert(nn.Module):
        def __init__(self):
            super().__init__()
            self.w1, self.w2, self.w3 = nn.Linear(H, I, bias=False), nn.Linear(I, H, bias=False), nn.Linear(H, I, bias=False)

    def skeleton():
        moe = nn.Module()
        moe.gate = nn.Linear(H, n_exp, bias=False)
        moe.experts = nn.ModuleList([Expert() for _ in range(n_exp)])
        layer = nn.Module()
        layer.block_sparse_moe = moe
        inner = nn.Module()
        inner.layers, inner.norm = nn.ModuleList([layer]), nn.LayerNorm(H, bias=False)
        top = nn.Module()
        top.model = inner
        return top.half().cuda()

    path = str(tmp_path / "per.gguf")
    dense = gguf_loader.load_into_model(skeleton(), path)
    packed = gguf_loader.load_into_model(skeleton(), path, packed=True)
    keep = gguf_loader.packed_expert_tensors(skeleton(), path)
    assert len(keep) == 3 * n_exp and keep["model.layers.0.block_sparse_moe.experts.2.w2"] == {
        "weight": ("blk.0.ffn_down_exps.weight", 11, 2)}
    assert sorted(packed.state_dict()) == ["model.layers.0.block_sparse_moe.gate.weight", "model.norm.weight"]
    for wname, (role, t) in types.items():
        mods = [getattr(ex, wname) for ex in packed.model.layers[0].block_sparse_moe.experts]
        assert all(type(m) is PackedLinear and m.q_type == t and m.row_src is None for m in mods)
        assert len({m.blocks.untyped_storage().data_ptr() for m in mods}) == 1  # one upload, three views
        assert [m.blocks.data_ptr() - mods[0].blocks.data_ptr() for m in mods] == [e * mods[0].blocks.numel() for e in range(n_exp)]
        for e, m in enumerate(mods):
            Wd = getattr(dense.model.layers[0].block_sparse_moe.experts[e], wname).weight.data
            assert torch.equal(i16(m.dense_weight()), i16(Wd)), (wname, e)
            for T in (3, 20):  # the GEMV and the tile kernel
                x = torch.randn(T, m.in_features, generator=torch.Generator().manual_seed(T + e)).half().cuda()
                y64 = x.double() @ Wd.double().T
                bound = 2.0 ** -11 * y64.abs() + m.in_features * 2.0 ** -23 * (x.double().abs() @ Wd.double().abs().T) + 2.0 ** -25
                assert bool(((m(x).double() - y64).abs() <= bound).all()), (wname, e, T)
