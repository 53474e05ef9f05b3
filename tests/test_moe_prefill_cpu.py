"""The packed MoE prefill, host side (no GPU): the route rule of include/gptq_gguf_moe_gemm.h stated in plain Python and
checked against torch's stable sort, the refusals of gq_moe_route and gq_linear_packed_experts (made before the first HIP
call, so host pointers do) in their documented order, the selection of PackedExperts between the decode path, the prefill
path and the loop with the ops calls replaced by dense fp32 math, and the combine both device paths share."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from test_moe_cpu import DenseOps, _packed_and_reference, _routing

torch = pytest.importorskip("torch")

A = 256  # any 16-byte aligned address, never dereferenced
F16, BF16 = 1, 2
BAD_TYPE, BAD_SHAPE, NULL = -1, -2, -6


# ------------------------------------------------------------------------------------------------ the route rule
def route_rule(ids, E):
    """The header's rule, literally: expert e's run holds the indices of the pairs that name e, ascending; the runs follow each
    other in expert order; an id outside [0, E) is in no run; -1 from the end of the last run on."""
    runs = [[p for p, e in enumerate(ids) if e == x] for x in range(E)]
    start = [0]
    for r in runs:
        start.append(start[-1] + len(r))
    order = [p for r in runs for p in r]
    return start, order + [-1] * (len(ids) - len(order))


def route_by_sort(ids, E):
    """The same from torch.sort(stable=True): ids int32 [P] on any device -> (expert_start int32 [E + 1], order int32 [P])."""
    valid = (ids >= 0) & (ids < E)
    key = torch.where(valid, ids, E).long()  # every pair without an expert behind the last run
    _, perm = torch.sort(key, stable=True)
    n = int(valid.sum())
    order = torch.where(torch.arange(ids.numel(), device=ids.device) < n, perm, -1).to(torch.int32)
    counts = torch.bincount(key, minlength=E + 1)[:E]
    start = torch.cat([torch.zeros(1, dtype=torch.long, device=ids.device), counts.cumsum(0)]).to(torch.int32)
    return start, order


ROUTE_INPUTS = {"mixed": (4, [2, 0, 4, 1, -1, 0, 2 ** 30, 2, 2, 0]),   # ids E, -1 and 2**30 among them; expert 3 is empty
                "one-expert": (3, [1] * 9),
                "none-valid": (2, [2, -1, 2 ** 30]),
                "single": (1, [0]),
                "descending": (5, [4, 3, 2, 1, 0, 4, 3, 2, 1, 0])}


@pytest.mark.parametrize("name", list(ROUTE_INPUTS))
def test_route_rule_is_the_stable_sort(name):
    E, ids = ROUTE_INPUTS[name]
    start, order = route_rule(ids, E)
    s2, o2 = route_by_sort(torch.tensor(ids, dtype=torch.int32), E)
    assert start == s2.tolist() and order == o2.tolist()
    assert len(start) == E + 1 and start[0] == 0 and start[-1] == sum(0 <= e < E for e in ids)
    for e in range(E):
        run = order[start[e]:start[e + 1]]
        assert run == sorted(run) and all(ids[p] == e for p in run)
    assert all(p == -1 for p in order[start[-1]:])
    if name == "mixed":
        assert start == [0, 3, 4, 7, 7] and order == [1, 5, 9, 3, 0, 7, 8, -1, -1, -1]


# ------------------------------------------------------------------------------------------------ header and binding
def test_moe_gemm_header_symbols_are_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi, ops
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_moe_gemm.h")).read()
    declared = set(re.findall(r"^int (gq_[a-z0-9_]+)\s*\(", hdr, re.M))
    L = _cabi.lib()
    assert declared == set(_cabi.EXPORTS_MOE_GEMM) == {"gq_moe_route", "gq_linear_packed_experts"}
    so = ctypes.CDLL(_cabi.SO_PATH)
    assert hasattr(so, "gq_moe_route") and hasattr(so, "gq_linear_packed_experts")
    assert len(L.gq_moe_route.argtypes) == 6 and len(L.gq_linear_packed_experts.argtypes) == 14
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6  # additive: the version stays
    assert '#include "gptq_gguf_moe.h"' in hdr
    pairs = int(re.search(r"#define GQ_MOE_ROUTE_MAX_PAIRS (\d+)", hdr).group(1))
    experts = int(re.search(r"#define GQ_MOE_ROUTE_MAX_EXPERTS (\d+)", hdr).group(1))
    assert pairs == _cabi.MOE_ROUTE_MAX_PAIRS == ops.MOE_ROUTE_MAX_PAIRS and pairs >= 2 ** 17
    assert experts == _cabi.MOE_ROUTE_MAX_EXPERTS == ops.MOE_ROUTE_MAX_EXPERTS and experts >= 256
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "gq_linear_packed_experts" in text and "gq_moe_route" in text, doc


# ------------------------------------------------------------------------------------------------ refusals
def test_moe_route_refusals_need_no_device():
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()

    def refused(status, word, pe=A, P=4, E=3, es=A, order=A):
        rc = L.gq_moe_route(pe, P, E, es, order, None)
        msg = L.gq_last_error().decode()
        assert rc == status and word in msg and "gq_moe_route" in msg, (rc, msg)

    for arg in ("pe", "es", "order"):
        refused(NULL, "is NULL", **{arg: None})
    refused(BAD_SHAPE, "E=0", E=0)
    refused(BAD_SHAPE, f"E={_cabi.MOE_ROUTE_MAX_EXPERTS + 1}", E=_cabi.MOE_ROUTE_MAX_EXPERTS + 1)
    refused(BAD_SHAPE, "E=-1", E=-1)
    refused(BAD_SHAPE, "P=0", P=0)
    refused(BAD_SHAPE, f"P={_cabi.MOE_ROUTE_MAX_PAIRS + 1}", P=_cabi.MOE_ROUTE_MAX_PAIRS + 1)
    refused(BAD_SHAPE, "pair_expert not 4-byte aligned", pe=A + 2)
    refused(BAD_SHAPE, "expert_start not 4-byte aligned", es=A + 1)
    refused(BAD_SHAPE, "order not 4-byte aligned", order=A + 2)
    # the order of the checks: NULL before E before P before the alignments; the limits themselves pass
    refused(NULL, "is NULL", order=None, E=0, P=0)
    refused(BAD_SHAPE, "E=0", E=0, P=0, pe=A + 2)
    refused(BAD_SHAPE, "P=0", P=0, pe=A + 2)
    refused(BAD_SHAPE, "order not 4-byte aligned", E=_cabi.MOE_ROUTE_MAX_EXPERTS, P=_cabi.MOE_ROUTE_MAX_PAIRS, order=A + 2)


def test_linear_packed_experts_refusals_need_no_device_and_come_in_the_documented_order():
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()

    def call(q_type=12, blocks=A, E=3, R=4, C=256, x=A, x_rows=2, ppr=2, es=A, order=A, n=4, x_dtype=F16, y=A):
        return L.gq_linear_packed_experts(q_type, blocks, E, R, C, x, x_rows, ppr, es, order, n, x_dtype, y, None)

    def refused(status, word, **kw):
        rc = call(**kw)
        msg = L.gq_last_error().decode()
        assert rc == status and word in msg and "gq_linear_packed_experts" in msg, (kw, rc, msg)

    for q_type in (3, 9, 15, 0):
        refused(BAD_TYPE, f"q_type {q_type}", q_type=q_type)
    refused(BAD_TYPE, "x_dtype 0", x_dtype=0)
    for arg in ("blocks", "x", "es", "order", "y"):
        refused(NULL, "is NULL", **{arg: None})
    refused(BAD_SHAPE, "E=0", E=0)
    refused(BAD_SHAPE, f"E={_cabi.MOE_ROUTE_MAX_EXPERTS + 1}", E=_cabi.MOE_ROUTE_MAX_EXPERTS + 1)
    refused(BAD_SHAPE, "R=0", R=0)
    refused(BAD_SHAPE, "P=0", n=0, x_rows=0)
    refused(BAD_SHAPE, "P=-1", n=-1)
    big = _cabi.MOE_ROUTE_MAX_PAIRS + 1
    refused(BAD_SHAPE, f"P={big}", n=big, x_rows=big, ppr=1)
    refused(BAD_SHAPE, "x_rows=3 * pairs_per_row=2 != P=4", x_rows=3)
    refused(BAD_SHAPE, "pairs_per_row=0", ppr=0)
    refused(BAD_SHAPE, "C=128", C=128)
    refused(BAD_SHAPE, "C=288", q_type=8, C=288)
    for q_type, bad, al in ((10, A + 2, 4), (11, A + 1, 2), (12, A + 8, 16), (13, A + 4, 16), (14, A + 3, 2), (8, A + 1, 2)):
        refused(BAD_SHAPE, f"blocks not {al}-byte aligned", q_type=q_type, blocks=bad)
    refused(BAD_SHAPE, "expert_start not 4-byte aligned", es=A + 2)
    refused(BAD_SHAPE, "order not 4-byte aligned", order=A + 2)
    refused(BAD_SHAPE, "x not 16-byte aligned", x=A + 8)
    refused(BAD_SHAPE, "y not 16-byte aligned", y=A + 2)
    # the documented order: every later fault is present too, the earliest one is named
    faults = [(BAD_TYPE, "q_type 9", dict(q_type=9)), (BAD_TYPE, "x_dtype 0", dict(x_dtype=0)), (NULL, "x is NULL", dict(x=None)),
              (BAD_SHAPE, "E=0", dict(E=0)), (BAD_SHAPE, "R=0", dict(R=0)), (BAD_SHAPE, "P=0", dict(n=0)),
              (BAD_SHAPE, "!= P=", dict(x_rows=3)), (BAD_SHAPE, "C=128", dict(C=128)), (BAD_SHAPE, "y not 16-byte aligned", dict(y=A + 2))]
    for i, (status, word, _) in enumerate(faults):
        kw = {}
        for _, _, later in faults[i:]:
            kw.update(later)
        refused(status, word, **kw)
    # the limits themselves pass the E and P rules: the refusal is a later check's
    refused(BAD_SHAPE, "y not 16-byte aligned", E=_cabi.MOE_ROUTE_MAX_EXPERTS, n=_cabi.MOE_ROUTE_MAX_PAIRS,
            x_rows=_cabi.MOE_ROUTE_MAX_PAIRS, ppr=1, y=A + 2)


def test_ops_refusals_name_the_value():
    from gptq_gguf_toolkit_amd import _cabi, ops
    E, R, C = 3, 4, 256
    blocks = torch.zeros(E * R * 144, dtype=torch.uint8)
    x = torch.zeros(2, C, dtype=torch.float16)

    def route(n, e=E):
        return torch.zeros(e + 1, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)

    for kw, word in ((dict(route=route(0)), "P=0"),
                     (dict(route=route(6)), r"x_rows=2 \* pairs_per_row=2 != P=6"),
                     (dict(route=route(4, e=2)), r"expert_start must be a contiguous int32 \[4\]"),
                     (dict(route=(route(4)[0], route(4)[1].long())), "order must be a contiguous int32"),
                     (dict(x=torch.zeros(2, 128, dtype=torch.float16)), "C=128"),
                     (dict(x=x.float()), "fp16 or bf16"),
                     (dict(E=ops.MOE_ROUTE_MAX_EXPERTS + 1), f"E={ops.MOE_ROUTE_MAX_EXPERTS + 1}"),
                     (dict(blocks=blocks[:-144]), "1728 contiguous uint8"),
                     (dict(), "CPU")):  # every argument good but on the host: there is no CPU path
        args = dict(q_type=12, blocks=blocks, E=E, R=R, x=x, route=route(4), pairs_per_row=2)
        args.update(kw)
        with pytest.raises(_cabi.GQError, match=word):
            ops.linear_packed_experts(**args)
    for args, word in (((torch.zeros(0, dtype=torch.int32), E), "P=0"),
                       ((torch.zeros(4, dtype=torch.int64), E), "int32"),
                       ((torch.zeros(4, dtype=torch.int32), 0), "E=0"),
                       ((torch.zeros(4, dtype=torch.int32), ops.MOE_ROUTE_MAX_EXPERTS + 1), "E=257"),
                       ((torch.zeros(ops.MOE_ROUTE_MAX_PAIRS + 1, dtype=torch.int32), E), f"P={ops.MOE_ROUTE_MAX_PAIRS + 1}"),
                       ((torch.zeros(4, dtype=torch.int32), E), "CPU")):
        with pytest.raises(_cabi.GQError, match=word):
            ops.moe_route(*args)


# ------------------------------------------------------------------------------------------------ PackedExperts selection
class PrefillOps(DenseOps):
    """test_moe_cpu.py's stand-ins plus the two calls of the prefill path: the route by torch's stable sort, the grouped
    GEMM as dense fp32 math on the pairs of the route; rows of pairs that are in no run are NaN."""

    def moe_route(self, pairs, E):
        assert pairs.dtype == torch.int32 and pairs.dim() == 1
        self.calls.append(("route", pairs.numel(), E))
        return route_by_sort(pairs, E)

    def linear_packed_experts(self, q_type, blocks, E, R, x, route, ppr):
        role, _ = self._role_of(blocks)
        start, order = route
        assert q_type == self.mod.levels[role][1] and x.shape[0] * ppr == order.numel() and start.numel() == E + 1
        self.calls.append(("prefill", role, order.numel(), ppr))
        y = torch.full((order.numel(), R), float("nan"))
        for e in range(E):
            for p in order[int(start[e]):int(start[e + 1])].tolist():
                y[p] = self.dense[role][e] @ x[p // ppr].float()
        return y

    def install(self, monkeypatch):
        from gptq_gguf_toolkit_amd import ops
        super().install(monkeypatch)
        monkeypatch.setattr(ops, "moe_route", self.moe_route)
        monkeypatch.setattr(ops, "linear_packed_experts", self.linear_packed_experts)
        return self


def kinds(fake):
    return {c[0] for c in fake.calls}


def test_packed_experts_selects_the_prefill_path_only_when_asked(monkeypatch):
    from gptq_gguf_toolkit_amd import GQError, ops
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts
    mod, dense, ref = _packed_and_reference()
    fake = PrefillOps(mod, dense).install(monkeypatch)
    E, K, H = mod.num_experts, 2, mod.hidden_dim

    def run(T, seed=None):
        del fake.calls[:]
        hidden = torch.randn(T, H, generator=torch.Generator().manual_seed(T)).half()
        idx, w = _routing(T, K, E, seed=100 + T if seed is None else seed, spare=3)
        return mod(hidden, idx, w), hidden, idx, w

    assert PackedExperts.prefill == "loop" and PackedExperts.prefill_max_pairs == 8192 <= ops.MOE_ROUTE_MAX_PAIRS
    run(17)
    assert kinds(fake) <= {"gemv", "gemm"} and not mod.takes_prefill_path(17, K)  # the default: the loop
    mod.prefill = "grouped"
    out, hidden, idx, w = run(17)
    assert fake.calls == [("route", 34, E), ("prefill", "gate", 34, K), ("prefill", "up", 34, K), ("prefill", "down", 34, 1)]
    assert mod.takes_prefill_path(17, K) and not mod.takes_decode_path(17, K)
    with torch.no_grad():
        want = ref(hidden.float(), idx, w)
    assert out.dtype == torch.float16 and out.shape == (17, H)
    assert bool(((out.float() - want).abs() <= 2.0 ** -11 * want.abs() + 1e-5).all())  # one rounding (the stand-ins' order: 1e-5)
    run(16)
    assert kinds(fake) == {"grouped"} and mod.takes_decode_path(16, K) and not mod.takes_prefill_path(16, K)
    mod.grouped_max_pairs = 0  # the decode path switched off: its inputs are prefill inputs
    run(1)
    assert kinds(fake) == {"route", "prefill"}
    del mod.grouped_max_pairs

    # a dense level falls back to the loop
    blocks, q = mod.levels["up"]
    mod.set_level("up", dense["up"].half(), None)
    run(17)
    assert not mod.takes_prefill_path(17, K) and kinds(fake) <= {"gemv", "gemm"} and len(fake.calls) > 0
    mod.set_level("up", blocks, q)

    # more experts than the route sorts by: the loop
    monkeypatch.setattr(ops, "MOE_ROUTE_MAX_EXPERTS", E - 1)
    run(17)
    assert kinds(fake) <= {"gemv", "gemm"}
    monkeypatch.setattr(ops, "MOE_ROUTE_MAX_EXPERTS", 256)

    # chunks: prefill_max_pairs = 8 with T = 10, K = 2 is three chunks of 4, 4 and 2 tokens with the unchunked result
    # (ten tokens are a decode step's by the default thresholds: that path is switched off here)
    mod.grouped_max_pairs = 0
    whole, hidden, idx, w = run(10)
    assert [c for c in fake.calls if c[0] == "route"] == [("route", 20, E)]
    mod.prefill_max_pairs = 8
    del fake.calls[:]
    parts = mod(hidden, idx, w)
    assert [c[1] for c in fake.calls if c[0] == "route"] == [8, 8, 4]
    assert [c[2] for c in fake.calls if c[0] == "prefill"] == [8] * 3 + [8] * 3 + [4] * 3
    assert torch.equal(parts, whole)
    mod.prefill_max_pairs = 10 ** 9  # capped by the kernel's limit
    monkeypatch.setattr(ops, "MOE_ROUTE_MAX_PAIRS", 6)
    del fake.calls[:]
    assert torch.equal(mod(hidden, idx, w), whole) and [c[1] for c in fake.calls if c[0] == "route"] == [6, 6, 6, 2]

    # a masked pair (id E) contributes nothing, as on the other paths
    del mod.prefill_max_pairs
    monkeypatch.setattr(ops, "MOE_ROUTE_MAX_PAIRS", 131072)
    idx2 = idx.clone()
    idx2[1, 1] = E
    a = mod(hidden, idx2, w)
    w1 = w.clone()
    w1[1, 1] = 0
    b = mod(hidden, idx, w1)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)

    del mod.grouped_max_pairs
    # instance settings leave the class alone
    assert PackedExperts.prefill == "loop" and PackedExperts.prefill_max_pairs == 8192
    assert PackedExperts(4, 256, 256).prefill == "loop"
    mod.prefill = "tiles"
    with pytest.raises(GQError, match="'loop' or 'grouped'"):
        mod(hidden, idx, w)


def test_install_experts_and_the_command_lines_carry_the_choice(tmp_path):
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralSparseMoeBlock
    from gptq_gguf_toolkit_amd import generate, gguf_loader, ppleval
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts, install_experts
    cfg = MixtralConfig(hidden_size=256, intermediate_size=512, num_local_experts=4, num_experts_per_tok=2,
                        num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2, vocab_size=32)

    def holder():
        h = torch.nn.Module()
        h.mlp = MixtralSparseMoeBlock(cfg).half()
        return h

    assert install_experts(holder(), ["mlp.experts"])["mlp.experts"].prefill == "loop"
    got = install_experts(holder(), ["mlp.experts"], prefill="grouped")["mlp.experts"]
    assert got.prefill == "grouped" and PackedExperts.prefill == "loop"
    with pytest.raises(ValueError, match="'loop' or 'grouped'"):
        install_experts(holder(), ["mlp.experts"], prefill="fast")
    with pytest.raises(ValueError, match="moe_prefill"):
        gguf_loader.load_into_model(holder(), "unused.gguf", packed=False, moe_prefill="grouped")
    ids = tmp_path / "ids.pt"
    torch.save([torch.zeros(1, 4, dtype=torch.long)], str(ids))
    base = ["--model_name_or_path", "m", "--output_file", "o.json"]
    for mod, extra in ((ppleval, ["--eval_datasets", str(ids)]), (generate, ["--prompt_ids", str(ids), "--max_new_tokens", "1"])):
        assert mod.parse_args(base + extra).moe_prefill == "loop"
        assert mod.parse_args(base + extra + ["--gguf", "f.gguf", "--packed", "--moe_prefill", "grouped"]).moe_prefill == "grouped"
        with pytest.raises(SystemExit):
            mod.parse_args(base + extra + ["--gguf", "f.gguf", "--moe_prefill", "grouped"])  # needs --packed


# ------------------------------------------------------------------------------------------------ the combine
@pytest.mark.parametrize("dt,u", [(torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)], ids=["f16", "bf16"])
def test_combine_is_the_fp32_sum_rounded_once_and_skips_masked_pairs(dt, u):
    """out = round(sum_k fp32(w[t, k]) * fp32(down[t K + k])), k ascending in fp32: against that sum kept in fp32 the only
    error is the final rounding to nearest, |diff| <= u |ref| (u = half an ulp: 2^-11 fp16, 2^-8 bf16; the magnitudes are
    chosen normal).  A masked pair contributes nothing even when its row of `down` is NaN."""
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts
    E, H, T, K = 4, 256, 9, 3
    mod = PackedExperts(E, H, 256, dt)
    g = torch.Generator().manual_seed(3)
    down = (torch.rand(T * K, H, generator=g) + 0.5).to(dt)
    w = torch.softmax(torch.randn(T, K, generator=g), -1).to(dt)
    pairs = torch.randint(0, E, (T * K,), generator=g).to(torch.int32)
    masked = [1, 5, 13, 26]
    for i, p in enumerate(masked):
        pairs[p] = (E, -1, 2 ** 30, E)[i]
        down[p] = float("nan")
    out = mod._combine(down, pairs, w)
    assert out.dtype == dt and out.shape == (T, H) and bool(torch.isfinite(out).all())
    ref = torch.zeros(T, H)
    for k in range(K):  # fp32, k ascending
        keep = torch.tensor([t * K + k not in masked for t in range(T)]).view(T, 1)
        ref = ref + torch.where(keep, down.view(T, K, H)[:, k].float() * w[:, k].float().unsqueeze(-1), torch.zeros(()))
    err = (out.double() - ref.double()).abs()
    print(f"{dt}: max |diff| / (u |ref|) = {float((err / (u * ref.double().abs())).max()):.3f}")
    assert float(ref.abs().min()) > 2.0 ** -14 and bool((err <= u * ref.double().abs()).all())
    alone = mod._combine(down, torch.full_like(pairs, E), w)  # every pair masked: zeros, not NaN
    assert bool((alone == 0).all())
