"""Error estimate of fused-expert units, host side (no GPU): the two gq_quad_form_experts symbols and every refusal of the
call with host pointers, and error_estimator.py's unit logic on the tiny Mixtral of tests/test_moe_quantize_cpu.py (2 layers,
E = 5 with a never-routed expert, H = 256, I = 512) with ops.h_accumulate / ops.quad_form / ops.quad_form_experts replaced by
torch-fp64 stand-ins: which units are scored, the common scale 2 / N of the expert Hessians, sum_e num_e / sum_e den_e, one
host read per unit, level order, the stand-in restored, the Linears untouched by the units next to them."""
import ctypes
import os
import re
import sys
import types

import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")
sys.path.insert(0, os.path.join(ROOT, "tests"))

REGEX = r".*layers.*((q|k|v|o|gate|up|down)_proj)$"  # the CLI's default
LEVELS = (("2.5625-Q2_K.pth", 1e-1), ("4.5-Q4_K.pth", 2e-2), ("6.5625-Q6_K.pth", 3e-3))  # (file, sigma / rms(W))
ROLES = ("gate_proj", "up_proj", "down_proj")


# ------------------------------------------------------------------------------------------------ the C ABI
def test_quad_form_experts_symbols_are_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_moe_errest.h")).read()
    declared = set(re.findall(r"\b(gq_[a-z0-9_]+)\s*\(", hdr))
    L = _cabi.lib()
    assert declared == set(_cabi.EXPORTS_MOE_ERREST) == {"gq_quad_form_experts", "gq_quad_form_experts_workspace_bytes"}
    assert not declared & set(_cabi.EXPORTS) and len(_cabi.EXPORTS) == 48  # gptq_gguf.h and its table keep their symbol set
    for sym in declared:
        assert hasattr(ctypes.CDLL(_cabi.SO_PATH), sym) and hasattr(L, sym), sym
        assert getattr(L, sym).argtypes, f"{sym} has no argtypes"
    assert int(re.search(r"#define GQ_QUAD_EXPERTS_MAX (\d+)", hdr).group(1)) == _cabi.QUAD_EXPERTS_MAX == 256
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6  # additive: the version stays
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`gq_quad_form_experts`" in doc and "`gq_quad_form_experts_workspace_bytes`" in doc


def test_quad_form_experts_argument_checks_need_no_device():
    """Every refusal comes before the first HIP call: a negative status and a message that names the argument."""
    from gptq_gguf_toolkit_amd import _cabi
    L, p, nul = _cabi.lib(), ctypes.c_void_p(256), ctypes.c_void_p(0)  # p: any 16-byte aligned address, never dereferenced
    big, S = 1 << 20, 4 * 256

    def call(A=p, a_dt=1, lda=256, sa=S, B=nul, b_dt=0, ldb=0, sb=0, H=p, E=3, R=4, C=256, out=p, ws=p, nws=big):
        return L.gq_quad_form_experts(A, a_dt, lda, sa, B, b_dt, ldb, sb, H, E, R, C, out, ws, nws, nul)

    def refused(rc, status, word):
        msg = L.gq_last_error().decode()
        assert rc == status and word in msg and msg.startswith("gq_quad_form_experts:"), (rc, msg)

    refused(call(A=nul), -6, "A is NULL")
    refused(call(H=nul), -6, "H is NULL")
    refused(call(out=nul), -6, "out is NULL")
    refused(call(a_dt=7), -1, "a_dtype")
    refused(call(B=p, b_dt=9, ldb=256, sb=S), -1, "b_dtype")
    refused(call(E=0), -2, "E=0")
    refused(call(E=257), -2, "E=257")
    refused(call(R=0), -2, "R=0")
    refused(call(C=192, lda=192), -2, "C=192")
    refused(call(E=256, R=1 << 30, C=1 << 20, lda=1 << 20, sa=1 << 50), -2, "2^31 tiles")
    refused(call(lda=128), -2, "lda=128")
    refused(call(B=p, b_dt=1, ldb=128, sb=S), -2, "ldb=128")
    refused(call(A=ctypes.c_void_p(258)), -2, "rows of A")
    refused(call(lda=260, sa=4 * 260), -2, "rows of A")  # 260 * 2 B = 520: not 16 k
    refused(call(B=ctypes.c_void_p(264), b_dt=0, ldb=256, sb=S), -2, "rows of B")
    refused(call(sa=S + 4), -2, "a_stride=1028")          # 1028 * 2 B: not 16 k
    refused(call(sa=S - 8), -2, "a_stride=1016")          # expert 1 would begin inside expert 0
    refused(call(B=p, b_dt=2, ldb=256, sb=S + 4), -2, "b_stride=1028")
    refused(call(H=ctypes.c_void_p(264)), -2, "H is not")
    refused(call(out=ctypes.c_void_p(260)), -2, "out / ws")
    refused(call(ws=nul, nws=0), -3, "workspace")
    refused(call(R=300, sa=300 * 256, nws=3 * 3 * 2 * 8 - 1), -3, "workspace")
    # E = 1 has no second expert: any stride
    refused(call(E=1, sa=3, ws=nul, nws=0), -3, "workspace")
    # one fp64 partial per (expert, 128-row tile, 128-column block); 0 for what the call refuses
    ws = L.gq_quad_form_experts_workspace_bytes
    assert ws(1, 1, 128) == 8 and ws(5, 257, 1280) == 5 * 3 * 10 * 8 and ws(256, 1, 128) == 256 * 8
    assert ws(0, 4, 256) == ws(257, 4, 256) == ws(3, 4, 192) == ws(3, 0, 256) == 0
    assert ws(1, 257, 1280) == L.gq_quad_form_workspace_bytes(257, 1280)


def test_ops_quad_form_experts_refuses_cpu_tensors():
    from gptq_gguf_toolkit_amd import _cabi, ops
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.quad_form_experts(torch.zeros(2, 4, 128), torch.zeros(2, 128, 128))


def test_tile_text_is_shared_by_both_kernels():
    """gq_quad_form and gq_quad_form_experts compile ONE tile: neither translation unit has a k loop of its own."""
    src = os.path.join(ROOT, "gptq-gguf-toolkit_amd", "csrc", "errest")
    core = open(os.path.join(src, "gq_quadform_core.hpp")).read()
    assert "qf_tile" in core and "__builtin_amdgcn_mfma_f32_32x32x2f32" in core and "qf_sum_partials" in core
    for f in ("gq_quadform.hip", "gq_quad_form_experts.hip"):
        text = open(os.path.join(src, f)).read()
        assert '#include "gq_quadform_core.hpp"' in text and "qf_tile<DTA, DTB, HAS_B>(" in text and "qf_sum_partials(" in text
        assert "mfma" not in text.replace("v_mfma_f32_32x32x2_f32", "") and "__launch_bounds__(QF_NT, 2)" in text
        assert "atomic" not in text.replace("std::atomic<bool> attr_set", "").replace("No atomics", "").lower()


# ------------------------------------------------------------------------------------------------ the driver
def _fix(H):
    H = H.double().clone()
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    return H


def _fp64_quad(A, H, B=None):
    D = (A.float() - B.float()).double() if B is not None else A.double()
    return ((D @ _fix(H)) * D).sum()


class _Counted(torch.Tensor):
    """What the stand-ins return: a tensor that counts the host reads made through it or its results."""
    reads = 0

    def item(self):
        _Counted.reads += 1
        return super().item()

    def tolist(self):
        _Counted.reads += 1
        return super().tolist()

    def cpu(self, *a, **k):
        _Counted.reads += 1
        return super().cpu(*a, **k)


def _fake_ops():
    me = types.SimpleNamespace(calls={"h_accumulate": 0, "quad_form": 0, "quad_form_experts": 0}, scales=set(), in_place=[])

    def h_accumulate(H, X, beta, alpha, ws=None):
        me.calls["h_accumulate"] += 1
        if H.dim() == 2 and H._base is not None and H._base.dim() == 3:  # a view of a stacked expert buffer
            me.scales.add((beta, alpha))
        x = X.double()
        H.copy_((H.double() * beta + alpha * (x.T @ x)).float())
        return H

    def quad_form(A, H, B=None, ws=None):
        me.calls["quad_form"] += 1
        return _fp64_quad(A, H, B).as_subclass(_Counted)

    def quad_form_experts(A, H, B=None, ws=None):
        me.calls["quad_form_experts"] += 1
        me.in_place.append(A.data_ptr())
        assert A.dim() == 3 and tuple(H.shape) == (A.shape[0], A.shape[2], A.shape[2]) and H.dtype == torch.float32
        return torch.stack([_fp64_quad(A[e], H[e], None if B is None else B[e]) for e in range(A.shape[0])]).as_subclass(_Counted)

    me.h_accumulate, me.quad_form, me.quad_form_experts = h_accumulate, quad_form, quad_form_experts
    return me


def _units(model):
    return [f"model.layers.{i}.mlp.experts.{r}" for i in range(len(model.model.layers)) for r in ROLES]


def _unit_weight(model, name):
    mod, _, role = name.rpartition(".")
    ex = model.get_submodule(mod)
    inter = ex.down_proj.shape[2]
    return {"gate_proj": ex.gate_up_proj.detach()[:, :inter], "up_proj": ex.gate_up_proj.detach()[:, inter:],
            "down_proj": ex.down_proj.detach()}[role]


def _write_db(model, db, names, weight_of):
    g = torch.Generator().manual_seed(5)
    for n in names:
        W = weight_of(n)
        os.makedirs(db / n)
        for f, s in LEVELS:
            torch.save((W + s * W.pow(2).mean().sqrt() * torch.randn(W.shape, generator=g)).contiguous(), str(db / n / f))


def _captured_expert_inputs(model, data):
    """{experts module: ({e: [x of w1 / w3, per call]}, {e: [x of w2]})} from pre-hooks on a CalibExperts of the test's own,
    in "loop" mode, and N, the calibration tokens; the model is left as it was."""
    from gptq_gguf_toolkit_amd import moe_calibration as mc
    out, hooks, installed = {}, [], []
    for i, layer in enumerate(model.model.layers):
        name = f"model.layers.{i}.mlp.experts"
        stand_in = mc.CalibExperts(layer.mlp.experts, "loop")
        installed.append((layer.mlp, "experts", layer.mlp.experts, name))
        layer.mlp.experts = stand_in
        xin, xmid = {}, {}
        out[name] = (xin, xmid)
        for e in range(stand_in.num_experts):
            ex = stand_in.expert(e)
            hooks.append(ex.w1.register_forward_pre_hook(lambda m, inp, d=xin, e=e: d.setdefault(e, []).append(inp[0].detach().clone())))
            hooks.append(ex.w2.register_forward_pre_hook(lambda m, inp, d=xmid, e=e: d.setdefault(e, []).append(inp[0].detach().clone())))
    n = 0
    with torch.no_grad():
        for _, kw in data:
            model(**kw)
            n += kw["input_ids"].numel()
    for h in hooks:
        h.remove()
    mc.restore(installed)
    return out, n


def _want_unit_error(W, xs, n_tokens, W_c):
    """sum_e num_e / sum_e den_e in fp64 with H_e = (2/N) sum x^T x (H_e = I where no token came)."""
    num = den = 0.0
    for e in range(W.shape[0]):
        C = W.shape[2]
        H = torch.zeros(C, C, dtype=torch.float64)
        for x in xs.get(e, []):
            H += (2.0 / n_tokens) * (x.double().T @ x.double())
        num += float(_fp64_quad(W[e], H, W_c[e]))
        den += float(_fp64_quad(W[e], H))
    return num / den


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from test_moe_quantize_cpu import calib, tiny_mixtral
    model = tiny_mixtral()
    data = [([], {"input_ids": ids}) for ids in calib(n=3)]
    db = tmp_path_factory.mktemp("moe_errest_db")
    linears = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and "self_attn" in n]
    _write_db(model, db, linears, lambda n: model.get_submodule(n).weight.detach())
    _write_db(model, db, _units(model), lambda n: _unit_weight(model, n))
    return model, data, db, linears


def _estimator(monkeypatch, model, data, db, regex=REGEX):
    import gptq_gguf_toolkit_amd.error_estimator as ee
    fake = _fake_ops()
    monkeypatch.setattr(ee, "_ops", fake)
    _Counted.reads = 0
    return ee, fake, ee.ErrorEstimator(model, data, regex, ["model.embed_tokens", "model.rotary_emb"], "model.layers",
                                       str(db), device="cpu")


def test_units_are_scored_with_one_scale_and_the_model_is_left_as_it_was(tiny, monkeypatch):
    """Fails without the feature: the estimator scores nn.Linear modules only and returns no unit."""
    model, data, db, linears = tiny
    experts = [layer.mlp.experts for layer in model.model.layers]
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    acts, n_tokens = _captured_expert_inputs(model, data)
    assert n_tokens == 3 * 64 and all(4 not in acts[m][0] and 2 <= len(acts[m][0]) < 5 for m in acts)  # never-routed experts

    ee, fake, est = _estimator(monkeypatch, model, data, db)
    errors = est.estimate()
    assert list(errors) == [-1] and sorted(errors[-1]) == sorted(linears + _units(model))
    assert all(layer.mlp.experts is m for layer, m in zip(model.model.layers, experts))  # restored, by identity
    assert all(torch.equal(p.detach(), before[n]) for n, p in model.named_parameters())
    # every expert Hessian is accumulated on a zeroed buffer with the SAME 2 / N
    assert fake.scales == {(1.0, 2.0 / n_tokens)}
    # per unit the denominator once and one numerator per level, grouped; ONE host read per unit and per Linear
    assert fake.calls["quad_form_experts"] == 6 * (1 + len(LEVELS)) and fake.calls["quad_form"] == len(linears) * (1 + len(LEVELS))
    assert _Counted.reads == 6 + len(linears)
    # the fused parameter is read in place: gate and down at the parameter's address, up inside gate_up_proj
    ptrs = {p.data_ptr() for m in experts for p in (m.gate_up_proj, m.down_proj)}
    ups = {m.gate_up_proj[:, 512:].data_ptr() for m in experts}
    assert set(fake.in_place) == ptrs | ups
    # 2 layers x (E per-expert Hessians for w1 / w3 + E for w2) + 2 layers x (q / k / v shared, o)
    assert est.hessians_built == 2 * 2 * 5 + 2 * 2
    for u in _units(model):
        assert est.levels[u] == [f for f, _ in LEVELS]
        mod, _, role = u.rpartition(".")
        xs = acts[mod][1 if role == "down_proj" else 0]
        W = _unit_weight(model, u)
        for (f, _), got in zip(LEVELS, errors[-1][u]):
            want = _want_unit_error(W, xs, n_tokens, torch.load(str(db / u / f)))
            assert abs(got - want) <= 1e-5 * want, (u, f, got, want)  # the stand-in keeps H in fp32
        assert errors[-1][u] == sorted(errors[-1][u], reverse=True)  # sigma falls as the level rises
    rep = ee.report(errors, est.levels)
    assert rep[_units(model)[0]] == [{"level": f[:-4], "error": e} for (f, _), e in zip(LEVELS, errors[-1][_units(model)[0]])]
    # group_by_numel: a unit counts E * R * C
    grouped = est.estimate(group_by_numel=True)
    assert set(grouped) == {256 * 256, 128 * 256, 5 * 512 * 256}
    assert sorted(grouped[5 * 512 * 256]) == sorted(_units(model))


def test_linears_are_scored_as_without_units_and_only_held_units_are_scored(tiny, monkeypatch, tmp_path):
    model, data, db, linears = tiny
    _, _, est = _estimator(monkeypatch, model, data, db)
    with_units = est.estimate()[-1]
    # a regex that names no unit: the estimator of before, no stand-in, the same values bit for bit
    ee, fake, est = _estimator(monkeypatch, model, data, db, regex=r".*layers.*((q|k|v|o)_proj)$")
    alone = est.estimate()[-1]
    assert sorted(alone) == sorted(linears) and fake.calls["quad_form_experts"] == 0
    assert fake.calls["h_accumulate"] == 2 * 2 * len(data) and not fake.scales  # q / k / v and o per block and sample: no expert
    assert all(alone[n] == with_units[n] for n in linears)
    # a database that holds one unit of one block only: that one is scored, its Hessian role alone is built
    part = tmp_path / "db"
    keep = "model.layers.1.mlp.experts.down_proj"
    os.makedirs(part)
    os.symlink(db / keep, part / keep)
    ee, fake, est = _estimator(monkeypatch, model, data, part, regex=r"experts\.(gate|up|down)_proj$")
    got = est.estimate()[-1]
    assert list(got) == [keep] and got[keep] == with_units[keep] and est.hessians_built == 5


def test_large_experts_take_the_per_expert_loop(tiny, monkeypatch):
    """Above GROUPED_MAX_TILES_PER_EXPERT tiles per expert a unit goes through ops.quad_form expert by expert: same values."""
    model, data, db, linears = tiny
    regex = r"layers\.0\.mlp\.experts\.(gate|down)_proj$"
    ee, fake, est = _estimator(monkeypatch, model, data, db, regex=regex)
    assert ee.GROUPED_MAX_TILES_PER_EXPERT == 1024  # profiles/quad_form_experts_rate.txt
    grouped = est.estimate()[-1]
    assert fake.calls == {"h_accumulate": fake.calls["h_accumulate"], "quad_form": 0, "quad_form_experts": 2 * (1 + len(LEVELS))}
    ee, fake, est = _estimator(monkeypatch, model, data, db, regex=regex)
    monkeypatch.setattr(ee, "GROUPED_MAX_TILES_PER_EXPERT", 4 * 2 - 1)  # an expert of this model has 4 x 2 tiles
    looped = est.estimate()[-1]
    assert fake.calls["quad_form_experts"] == 0 and fake.calls["quad_form"] == 2 * 5 * (1 + len(LEVELS))
    assert sorted(looped) == sorted(grouped) and all(looped[u] == grouped[u] for u in grouped)
    assert _Counted.reads == 2  # still one host read per unit


def test_a_module_that_cannot_be_adapted_is_left_alone(monkeypatch, tmp_path):
    """Non-SiLU experts are not scored (and not refused: the Linears next to them are scored as before)."""
    from test_moe_quantize_cpu import calib, tiny_mixtral
    model = tiny_mixtral(hidden_act="gelu")
    data = [([], {"input_ids": ids}) for ids in calib(n=1)]
    linears = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and "self_attn" in n]
    _write_db(model, tmp_path, linears[:1], lambda n: model.get_submodule(n).weight.detach())
    _write_db(model, tmp_path, _units(model)[:1], lambda n: _unit_weight(model, n))
    _, fake, est = _estimator(monkeypatch, model, data, tmp_path)
    with pytest.raises(FileNotFoundError):  # as before: a Linear the regex names must be in the database
        est.estimate()
    _, fake, est = _estimator(monkeypatch, model, data, tmp_path, regex=r"layers\.0\.(self_attn\.q_proj|mlp\.experts\.gate_proj)$")
    assert list(est.estimate()[-1]) == linears[:1] and fake.calls["quad_form_experts"] == 0


def test_packed_resident_store_stays_refused():
    from gptq_gguf_toolkit_amd.error_estimator import ErrorEstimator
    with pytest.raises(ValueError, match="packed-resident"):
        ErrorEstimator(None, [], REGEX, [], "model.layers", "db", level_store=types.SimpleNamespace(resident="packed"))
