"""The packed MoE path, host side (no GPU): the additive header include/gptq_gguf_moe.h and its binding, the refusals of
gq_gemv_packed_experts (made before the first HIP call, so host pointers do) and of ops.gemv_packed_experts, the loader's
names and stacking of merged expert tensors in both layouts (a spec-written file of F16 tensors), and the routing of
PackedExperts between the grouped launches and the per-expert loop with the ops calls replaced by dense fp32 math."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")

P = 256  # any 16-byte aligned address, never dereferenced
F16, BF16 = 1, 2
BAD_TYPE, BAD_SHAPE, NULL = -1, -2, -6


# ------------------------------------------------------------------------------------------------ header and binding
def test_moe_header_symbol_is_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi, ops
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_moe.h")).read()
    declared = set(re.findall(r"^int (gq_[a-z0-9_]+)\s*\(", hdr, re.M))
    L = _cabi.lib()
    assert declared == set(_cabi.EXPORTS_MOE) == {"gq_gemv_packed_experts"}
    assert hasattr(ctypes.CDLL(_cabi.SO_PATH), "gq_gemv_packed_experts") and len(L.gq_gemv_packed_experts.argtypes) == 13
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6 and len(_cabi.EXPORTS) == 48  # additive: the version stays
    assert '#include "gptq_gguf_qgemv.h"' in hdr
    assert int(re.search(r"#define GQ_MOE_MAX_PAIRS (\d+)", hdr).group(1)) == _cabi.MOE_MAX_PAIRS == ops.MOE_MAX_PAIRS == 64
    for word in ("BIT FOR BIT", "is skipped", "multiple of that alignment", "never read by the host"):
        assert word in hdr, word
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "gq_gemv_packed_experts" in text, doc


def test_gemv_packed_experts_refusals_need_no_device():
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()

    def call(q_type=12, blocks=P, E=3, R=4, C=256, x=P, x_rows=2, pe=P, n=4, ppr=2, x_dtype=F16, y=P):
        return L.gq_gemv_packed_experts(q_type, blocks, E, R, C, x, x_rows, pe, n, ppr, x_dtype, y, None)

    def refused(status, word, **kw):
        rc = call(**kw)
        msg = L.gq_last_error().decode()
        assert rc == status and word in msg and "gq_gemv_packed_experts" in msg, (kw, rc, msg)

    refused(BAD_SHAPE, "P=0", n=0, x_rows=0)
    refused(BAD_SHAPE, "P=65", n=65, x_rows=65, ppr=1)
    refused(BAD_SHAPE, "P=-1", n=-1)
    refused(BAD_SHAPE, "x_rows=3 * pairs_per_row=2 != P=4", x_rows=3)
    refused(BAD_SHAPE, "pairs_per_row=0", ppr=0)
    refused(BAD_SHAPE, "x_rows=0", x_rows=0)
    refused(BAD_SHAPE, "C=128", C=128)
    refused(BAD_SHAPE, "C=288", q_type=8, C=288)
    refused(BAD_SHAPE, "R=0", R=0)
    refused(BAD_SHAPE, "E=0", E=0)
    refused(BAD_SHAPE, "E=65536", E=65536)
    refused(BAD_TYPE, "x_dtype 0", x_dtype=0)
    for q_type in (3, 9, 15, 0):
        refused(BAD_TYPE, f"q_type {q_type}", q_type=q_type)
    for q_type, bad, al in ((10, P + 2, 4), (11, P + 1, 2), (12, P + 8, 16), (13, P + 4, 16), (14, P + 3, 2), (8, P + 1, 2)):
        refused(BAD_SHAPE, f"blocks not {al}-byte aligned", q_type=q_type, blocks=bad)
    refused(BAD_SHAPE, "pair_expert not 4-byte aligned", pe=P + 2)
    refused(BAD_SHAPE, "x not 16-byte aligned", x=P + 8)
    refused(BAD_SHAPE, "y not 16-byte aligned", y=P + 2)
    for arg in ("blocks", "x", "pe", "y"):
        refused(NULL, "is NULL", **{arg: None})
    # P = 64 is the last P that passes the P rule: the refusal is the next check's
    refused(BAD_SHAPE, "y not 16-byte aligned", n=64, x_rows=64, ppr=1, y=P + 2)
    refused(BAD_SHAPE, "y not 16-byte aligned", E=65535, y=P + 2)


def test_gemv_packed_experts_names_the_earlier_of_two_faults():
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()
    for status, word, kw in ((BAD_TYPE, "q_type 9", dict(q_type=9, x=None)),
                             (BAD_TYPE, "x_dtype 0", dict(x_dtype=0, blocks=None)),
                             (NULL, "x is NULL", dict(x=None, C=128)),
                             (BAD_SHAPE, "R=0 (not in [1, 2^31))", dict(R=0, C=128)),
                             (BAD_SHAPE, "C=128 (C % 256 != 0 or not in [256, 2^31); Q8_0 and IQ4_NL included)", dict(C=128, y=P + 2)),
                             (BAD_SHAPE, "blocks not 16-byte aligned", dict(blocks=P + 8, x=P + 8))):
        args = dict(q_type=12, blocks=P, E=3, R=4, C=256, x=P, x_rows=2, pe=P, n=4, ppr=2, x_dtype=F16, y=P)
        args.update(kw)
        rc = L.gq_gemv_packed_experts(args["q_type"], args["blocks"], args["E"], args["R"], args["C"], args["x"], args["x_rows"],
                                      args["pe"], args["n"], args["ppr"], args["x_dtype"], args["y"], None)
        msg = L.gq_last_error().decode()
        assert rc == status and msg.startswith("gq_gemv_packed_experts: ") and word in msg, (kw, rc, msg)


def test_ops_gemv_packed_experts_refusals_name_the_value():
    from gptq_gguf_toolkit_amd import _cabi, ops
    E, R, C = 3, 4, 256
    blocks = torch.zeros(E * R * 144, dtype=torch.uint8)
    x = torch.zeros(2, C, dtype=torch.float16)

    def pe(n):
        return torch.zeros(n, dtype=torch.int32)

    for kw, word in ((dict(pair_expert=pe(0)), "P=0"),
                     (dict(pair_expert=pe(65)), "P=65"),
                     (dict(pair_expert=pe(6)), r"x_rows=2 \* pairs_per_row=2 != P=6"),
                     (dict(x=torch.zeros(2, 128, dtype=torch.float16)), "C=128"),
                     (dict(x=x.float()), "fp16 or bf16"),
                     (dict(pair_expert=pe(4).long()), "int32"),
                     (dict(blocks=blocks[:-144]), "1728 contiguous uint8"),
                     (dict(), "CPU")):  # every argument good but on the host: there is no CPU path
        args = dict(q_type=12, blocks=blocks, E=E, R=R, x=x, pair_expert=pe(4), pairs_per_row=2)
        args.update(kw)
        with pytest.raises(_cabi.GQError, match=word):
            ops.gemv_packed_experts(**args)


# ------------------------------------------------------------------------------------------------ the loader
E_, I_, H_ = 3, 8, 4


def _moe_file(tmp_path, drop=()):
    from gguf_spec_writer import serialise
    rng = np.random.default_rng(5)
    t = {"blk.0.ffn_gate_inp.weight": ((E_, H_), "F32", rng.standard_normal((E_, H_)).astype(np.float32)),
         "blk.0.ffn_gate_exps.weight": ((E_, I_, H_), "F16", rng.standard_normal((E_, I_, H_)).astype(np.float16)),
         "blk.0.ffn_down_exps.weight": ((E_, H_, I_), "F16", rng.standard_normal((E_, H_, I_)).astype(np.float16)),
         "blk.0.ffn_up_exps.weight": ((E_, I_, H_), "F16", rng.standard_normal((E_, I_, H_)).astype(np.float16)),
         "output_norm.weight": ((H_,), "F32", rng.standard_normal(H_).astype(np.float32))}
    for name in drop:
        del t[name]
    path = tmp_path / "moe.gguf"
    path.write_bytes(serialise([("general.architecture", "str", "llama"), ("llama.expert_count", "u32", E_)],
                               [(n, shape, kind, a.tobytes()) for n, (shape, kind, a) in t.items()]))
    return str(path), {n: torch.from_numpy(a) for n, (_, _, a) in t.items()}


def test_loader_names_and_stacks_merged_expert_tensors_in_both_layouts(tmp_path):
    from gptq_gguf_toolkit_amd import gguf_loader
    path, t = _moe_file(tmp_path)
    gate, up, down = (t[f"blk.0.ffn_{r}_exps.weight"] for r in ("gate", "up", "down"))

    fused = list(gguf_loader.iter_gguf_tensors(path, "cpu"))
    assert [n for n, _ in fused] == ["model.layers.0.mlp.gate.weight", "model.layers.0.mlp.experts.down_proj",
                                     "model.layers.0.mlp.experts.gate_up_proj", "model.norm.weight"]  # gate_up: where up stands
    sd = dict(fused)
    assert set(gguf_loader.load_state_dict(path, "cpu")) == set(sd)  # the fused layout is the default
    gu = sd["model.layers.0.mlp.experts.gate_up_proj"]
    assert gu.shape == (E_, 2 * I_, H_) and gu.dtype == torch.float16
    for e in range(E_):
        assert torch.equal(gu[e], torch.cat([gate[e], up[e]]))
    assert torch.equal(sd["model.layers.0.mlp.experts.down_proj"], down)
    assert torch.equal(sd["model.layers.0.mlp.gate.weight"], t["blk.0.ffn_gate_inp.weight"])

    per = gguf_loader.load_state_dict(path, "cpu", torch.float32, expert_layout="per_expert")
    want = ["model.layers.0.block_sparse_moe.gate.weight"]
    want += [f"model.layers.0.block_sparse_moe.experts.{e}.{w}.weight" for w in ("w1", "w2", "w3") for e in range(E_)]
    assert list(per) == want + ["model.norm.weight"]
    for e in range(E_):
        pre = f"model.layers.0.block_sparse_moe.experts.{e}."
        assert per[pre + "w1.weight"].dtype == torch.float32
        assert torch.equal(per[pre + "w1.weight"], gate[e].float()) and torch.equal(per[pre + "w3.weight"], up[e].float())
        assert torch.equal(per[pre + "w2.weight"], down[e].float())

    raw = dict(gguf_loader.iter_gguf_tensors(path, "cpu", hf_layout=False))
    assert list(raw) == list(t) and raw["blk.0.ffn_gate_exps.weight"].shape == (E_, I_, H_)
    assert all(torch.equal(raw[n], t[n]) for n in t)

    assert gguf_loader.expert_tensor("blk.12.ffn_up_exps.weight") == (12, "up", "w3")
    assert gguf_loader.expert_tensor("blk.0.ffn_up.weight") is None
    with pytest.raises(ValueError, match="expert_layout"):
        next(gguf_loader.iter_gguf_tensors(path, "cpu", expert_layout="stacked"))


def test_loader_refuses_half_of_a_fused_parameter(tmp_path):
    from gptq_gguf_toolkit_amd import gguf_loader
    path, _ = _moe_file(tmp_path, drop=("blk.0.ffn_gate_exps.weight",))
    with pytest.raises(NotImplementedError, match="ffn_up_exps.*no ffn_gate_exps"):
        list(gguf_loader.iter_gguf_tensors(path, "cpu"))
    assert len(gguf_loader.load_state_dict(path, "cpu", expert_layout="per_expert")) == 2 + 2 * E_  # no fusing: nothing to refuse


def test_load_into_model_takes_the_layout_from_the_model(tmp_path):
    """The same file into a model with per-expert Linears and into one with fused 3-D parameters."""
    from gptq_gguf_toolkit_amd import gguf_loader
    import torch.nn as nn
    path, t = _moe_file(tmp_path)

    def skeleton(moe_name, moe):
        layer = nn.Module()
        setattr(layer, moe_name, moe)
        inner = nn.Module()
        inner.layers = nn.ModuleList([layer])
        inner.norm = nn.LayerNorm(H_, bias=False)
        top = nn.Module()
        top.model = inner
        return top.half()

    class Expert(nn.Module):
        def __init__(self):
            super().__init__()
            self.w1, self.w2, self.w3 = nn.Linear(H_, I_, bias=False), nn.Linear(I_, H_, bias=False), nn.Linear(H_, I_, bias=False)

    moe = nn.Module()
    moe.gate = nn.Linear(H_, E_, bias=False)
    moe.experts = nn.ModuleList([Expert() for _ in range(E_)])
    per = skeleton("block_sparse_moe", moe)
    assert gguf_loader.expert_layout_of(per) == "per_expert"
    gguf_loader.load_into_model(per, path)
    assert torch.equal(per.model.layers[0].block_sparse_moe.experts[2].w2.weight, t["blk.0.ffn_down_exps.weight"][2])

    mlp = nn.Module()
    mlp.gate = nn.Linear(H_, E_, bias=False)
    mlp.experts = nn.Module()
    mlp.experts.gate_up_proj = nn.Parameter(torch.zeros(E_, 2 * I_, H_))
    mlp.experts.down_proj = nn.Parameter(torch.zeros(E_, H_, I_))
    fused = skeleton("mlp", mlp)
    assert gguf_loader.expert_layout_of(fused) == "fused"
    gguf_loader.load_into_model(fused, path)
    assert torch.equal(fused.model.layers[0].mlp.experts.gate_up_proj[1, I_:], t["blk.0.ffn_up_exps.weight"][1])
    assert gguf_loader.packed_expert_tensors(fused, path) == {}  # F16 tensors (and H % 256 != 0): nothing stays packed


# ------------------------------------------------------------------------------------------------ PackedExperts routing
class DenseOps:
    """The five ops calls PackedExperts makes, as dense fp32 math on the weights a test registered for its block tensors;
    every call is recorded."""

    def __init__(self, mod, dense):
        self.mod, self.dense, self.calls = mod, dense, []

    def _role_of(self, blocks):
        for role, (b, _) in self.mod.levels.items():
            if blocks.untyped_storage().data_ptr() == b.untyped_storage().data_ptr():
                return role, (blocks.data_ptr() - b.data_ptr()) // (b.numel() // self.mod.num_experts)
        raise AssertionError("blocks of no level")

    def gemv_packed_experts(self, q_type, blocks, E, R, x, pairs, ppr):
        role, _ = self._role_of(blocks)
        assert q_type == self.mod.levels[role][1] and pairs.dtype == torch.int32 and x.shape[0] * ppr == pairs.numel()
        self.calls.append(("grouped", role, pairs.numel(), ppr))
        W = self.dense[role]
        y = torch.full((pairs.numel(), R), float("nan"))
        for p, e in enumerate(pairs.tolist()):
            if 0 <= e < E:
                y[p] = W[e] @ x[p // ppr].float()
        return y

    def _one(self, kind):
        def fn(q_type, blocks, x, row_src=None):
            role, e = self._role_of(blocks)
            assert row_src is None and q_type == self.mod.levels[role][1]
            self.calls.append((kind, role, e, x.shape[0]))
            return x.float() @ self.dense[role][e].T
        return fn

    def install(self, monkeypatch):
        from gptq_gguf_toolkit_amd import ops
        monkeypatch.setattr(ops, "gemv_packed_experts", self.gemv_packed_experts)
        monkeypatch.setattr(ops, "gemv_packed", self._one("gemv"))
        monkeypatch.setattr(ops, "linear_packed", self._one("gemm"))
        monkeypatch.setattr(ops, "fwd_silu_mul", lambda g, u: torch.nn.functional.silu(g.float()) * u.float())
        return self


def _packed_and_reference(E=4, H=256, I=256):
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts
    g = torch.Generator().manual_seed(11)
    dense = {"gate": torch.randn(E, I, H, generator=g) * 0.05, "up": torch.randn(E, I, H, generator=g) * 0.05,
             "down": torch.randn(E, H, I, generator=g) * 0.05}
    mod = PackedExperts(E, H, I)
    for role, (q, ts) in zip(("gate", "up", "down"), ((12, 144), (13, 176), (14, 210))):  # a type per role
        mod.set_level(role, torch.zeros(E * dense[role].shape[1] * (dense[role].shape[2] // 256) * ts, dtype=torch.uint8), q)
    ref = MixtralExperts(MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=2,
                                       num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2, vocab_size=32))
    with torch.no_grad():
        ref.gate_up_proj.copy_(torch.cat([dense["gate"], dense["up"]], dim=1))
        ref.down_proj.copy_(dense["down"])
    return mod, dense, ref.float()


def _routing(T, K, E, seed, spare):
    """top-K of random logits over the experts except `spare`, which no token names."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(T, E, generator=g)
    logits[:, spare] = -1e9
    w, idx = torch.topk(torch.softmax(logits, -1), K, -1)
    return idx, w / w.sum(-1, keepdim=True)


@pytest.mark.parametrize("T", [1, 5, 16, 17, 40])
def test_packed_experts_paths_and_result(monkeypatch, T):
    """fp32 stand-ins for the kernels, fp16 in and out.  Against MixtralExperts.forward on the same weights and the same
    (fp16) hidden states in fp32: the decode path rounds once (|diff| <= 2^-11 |ref|), the loop path rounds each of the K
    terms to fp16 and adds them in fp16 (index_add_), at most 2^-11 (|term| + |partial sum|) per step <= 3 * 2^-11 * sum_k
    |term_k| for K = 2; 1e-5 covers the fp32 summation orders of the stand-ins."""
    from gptq_gguf_toolkit_amd import ops
    mod, dense, ref = _packed_and_reference()
    fake = DenseOps(mod, dense).install(monkeypatch)
    E, K, H = mod.num_experts, 2, mod.hidden_dim
    hidden = torch.randn(T, H, generator=torch.Generator().manual_seed(T)).half()
    idx, w = _routing(T, K, E, seed=100 + T, spare=3)
    assert mod.gemv_max_t == ops.GEMV_MAX_T == 16 and mod.grouped_max_pairs == ops.MOE_MAX_PAIRS == 64
    out = mod(hidden, idx, w)
    with torch.no_grad():
        want = ref(hidden.float(), idx, w)
        terms = torch.stack([torch.stack([(dense["down"][e] @ (torch.nn.functional.silu(dense["gate"][e] @ h) * (dense["up"][e] @ h)))
                                          for e in row]) for row, h in zip(idx.tolist(), hidden.float())]) * w.unsqueeze(-1)
    assert out.dtype == torch.float16 and out.shape == (T, H)
    grouped = T <= 16
    assert mod.takes_decode_path(T, K) == grouped
    if grouped:
        assert fake.calls == [("grouped", "gate", T * K, K), ("grouped", "up", T * K, K), ("grouped", "down", T * K, 1)]
        bound = 2.0 ** -11 * want.abs() + 1e-5
    else:
        assert {c[0] for c in fake.calls} <= {"gemv", "gemm"}
        assert 3 not in {c[2] for c in fake.calls} and {c[2] for c in fake.calls} == set(idx.unique().tolist())  # never the spare
        for kind, role, e, n in fake.calls:
            assert n == int((idx == e).sum()) and kind == ("gemv" if n <= 16 else "gemm")
        bound = 3 * 2.0 ** -11 * terms.abs().sum(1) + 1e-5
    err = (out.float() - want).abs()
    print(f"T={T}: max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


def test_packed_experts_thresholds_and_refusals(monkeypatch):
    from gptq_gguf_toolkit_amd import GQError
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts
    mod, dense, _ = _packed_and_reference()
    fake = DenseOps(mod, dense).install(monkeypatch)
    K = 2

    def path(T, **attrs):
        for k, v in attrs.items():
            setattr(mod, k, v)
        del fake.calls[:]
        idx, w = _routing(T, K, mod.num_experts, seed=T, spare=0)
        mod(torch.zeros(T, mod.hidden_dim, dtype=torch.float16), idx, w)
        kinds = {c[0] for c in fake.calls}
        assert kinds == {"grouped"} or "grouped" not in kinds
        return "grouped" if kinds == {"grouped"} else "loop"

    assert [path(T) for T in (1, 16, 17)] == ["grouped", "grouped", "loop"]
    assert [path(T, grouped_max_pairs=8) for T in (4, 5)] == ["grouped", "loop"]          # T * K <= 8
    assert [path(T, grouped_max_pairs=64, gemv_max_t=3) for T in (3, 4)] == ["grouped", "loop"]
    assert path(1, grouped_max_pairs=0, gemv_max_t=16) == "loop"                          # 0 switches the decode path off
    assert path(1, grouped_max_pairs=1000, gemv_max_t=1000) == "grouped" and path(33) == "loop"  # the kernels' limits hold
    assert PackedExperts.grouped_max_pairs == 64 and PackedExperts.gemv_max_t == 16       # instances only

    mod.grouped_max_pairs, mod.gemv_max_t = 64, 16
    # a masked pair (id E, transformers' convention) contributes nothing on either path
    idx, w = _routing(4, K, mod.num_experts, seed=9, spare=0)
    idx2 = idx.clone()
    idx2[1, 1] = mod.num_experts
    h = torch.randn(4, mod.hidden_dim, generator=torch.Generator().manual_seed(2)).half()
    a = mod(h, idx2, w)
    mod.grouped_max_pairs = 0
    b = mod(h, idx2, w)
    assert bool(torch.isfinite(a).all()) and float((a.float() - b.float()).abs().max()) <= 1e-2 * float(b.abs().max())
    w1 = w.clone()
    w1[1, 1] = 0
    c = mod(h, idx, w1)  # the same as that pair with weight 0 (another gather: fp16 rounding apart)
    assert float((c.float() - b.float()).abs().max()) <= 1e-2 * float(b.abs().max())

    with pytest.raises(GQError, match="float16"):
        mod(h.float(), idx, w)
    with pytest.raises(GQError, match="no up level"):
        fresh = PackedExperts(4, 256, 256)
        fresh.set_level("gate", mod.levels["gate"][0], 12)
        fresh(h, idx, w)
    with pytest.raises(GQError, match="147456 contiguous uint8"):
        PackedExperts(4, 256, 256).set_level("down", torch.zeros(10, dtype=torch.uint8), 12)
    with pytest.raises(GQError, match="dense level"):
        PackedExperts(4, 256, 256).set_level("down", torch.zeros(4, 256, 256), None)
    with pytest.raises(TypeError, match="fp16 or bf16"):
        PackedExperts(4, 256, 256, torch.float32)
    assert "gate_q_type=12, up_q_type=13, down_q_type=14" in repr(mod)
    assert mod.gate_up_proj.is_meta and mod.gate_up_proj.shape == (4, 512, 256) and mod.down_proj.shape == (4, 256, 256)
    assert not list(mod.parameters())


def test_replace_experts_swaps_a_mixtral_experts_module():
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralSparseMoeBlock
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts, experts_shaped, install_experts
    cfg = MixtralConfig(hidden_size=256, intermediate_size=512, num_local_experts=4, num_experts_per_tok=2,
                        num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2, vocab_size=32)
    holder = torch.nn.Module()
    holder.mlp = MixtralSparseMoeBlock(cfg).half()
    assert experts_shaped(holder.mlp.experts) and not experts_shaped(holder.mlp.gate)
    mods = install_experts(holder, ["mlp.experts"])
    got = holder.mlp.experts
    assert mods == {"mlp.experts": got} and isinstance(got, PackedExperts)
    assert (got.num_experts, got.hidden_dim, got.intermediate_dim, got.dtype) == (4, 256, 512, torch.float16)
    assert [n for n, _ in holder.named_parameters()] == ["mlp.gate.weight"]
    with pytest.raises(TypeError, match="gate_up_proj"):
        install_experts(holder, ["mlp.gate"])
