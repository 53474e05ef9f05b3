"""Layer error estimator, host side (no GPU): the two gq_quad_form symbols and their argument checks, the reference's own
three floats (fixture G18, tests/golden/make_golden_errest.py) against the fp64 expression, and error_estimator.py's host
logic on the tiny Llama with ops.quad_form / ops.h_accumulate replaced by torch-fp64 stand-ins: Hessian sharing, level
order, one host read per Linear, the refusals, the CLI's arguments and JSON shape."""
import ctypes
import json
import os
import re
import sys
import types

import numpy as np
import pytest

from conftest import ROOT, load_golden

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_quad_form_symbols_are_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_errest.h")).read()
    declared = set(re.findall(r"\b(gq_[a-z0-9_]+)\s*\(", hdr))
    L = _cabi.lib()
    assert declared == set(_cabi.EXPORTS_ERREST) == {"gq_quad_form", "gq_quad_form_workspace_bytes"}
    assert not declared & set(_cabi.EXPORTS)  # gptq_gguf.h and its table keep their symbol set
    for sym in declared:
        assert hasattr(ctypes.CDLL(_cabi.SO_PATH), sym) and hasattr(L, sym), sym
        assert getattr(L, sym).argtypes, f"{sym} has no argtypes"
    assert "evopress/src/error_estimator.py:88-103" in hdr
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6  # additive: the version stays
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`gq_quad_form`" in doc and "`gq_quad_form_workspace_bytes`" in doc


def test_quad_form_argument_checks_need_no_device():
    """Every refusal comes before the first HIP call: a negative status and a message that names the argument."""
    from gptq_gguf_toolkit_amd import _cabi
    L, p, nul = _cabi.lib(), ctypes.c_void_p(256), ctypes.c_void_p(0)  # p: any 16-byte aligned address, never dereferenced

    def refused(rc, status, word):
        msg = L.gq_last_error().decode()
        assert rc == status and word in msg, (rc, msg)

    big = 1 << 20
    refused(L.gq_quad_form(nul, 1, 256, nul, 0, 0, p, 4, 256, p, p, big, nul), -6, "A is NULL")
    refused(L.gq_quad_form(p, 1, 256, nul, 0, 0, nul, 4, 256, p, p, big, nul), -6, "H is NULL")
    refused(L.gq_quad_form(p, 1, 256, nul, 0, 0, p, 4, 256, nul, p, big, nul), -6, "out is NULL")
    refused(L.gq_quad_form(p, 7, 256, nul, 0, 0, p, 4, 256, p, p, big, nul), -1, "a_dtype")
    refused(L.gq_quad_form(p, 1, 256, p, 9, 256, p, 4, 256, p, p, big, nul), -1, "b_dtype")
    refused(L.gq_quad_form(p, 1, 192, nul, 0, 0, p, 4, 192, p, p, big, nul), -2, "C=192")
    refused(L.gq_quad_form(p, 1, 256, nul, 0, 0, p, 0, 256, p, p, big, nul), -2, "R=0")
    refused(L.gq_quad_form(p, 1, 128, nul, 0, 0, p, 4, 256, p, p, big, nul), -2, "lda=128")
    refused(L.gq_quad_form(ctypes.c_void_p(258), 1, 256, nul, 0, 0, p, 4, 256, p, p, big, nul), -2, "rows of A")
    refused(L.gq_quad_form(p, 1, 260, nul, 0, 0, p, 4, 256, p, p, big, nul), -2, "rows of A")  # 260 * 2 B = 520: not 16 k
    refused(L.gq_quad_form(p, 1, 256, ctypes.c_void_p(264), 0, 256, p, 4, 256, p, p, big, nul), -2, "rows of B")
    refused(L.gq_quad_form(p, 1, 256, nul, 0, 0, p, 4, 256, p, nul, 0, nul), -3, "workspace")
    refused(L.gq_quad_form(p, 1, 256, nul, 0, 0, p, 300, 256, p, p, 8, nul), -3, "workspace")
    # one fp64 partial per (128-row tile, 128-column block)
    assert L.gq_quad_form_workspace_bytes(1, 128) == 8
    assert L.gq_quad_form_workspace_bytes(257, 1280) == 3 * 10 * 8
    assert L.gq_quad_form_workspace_bytes(4, 192) == 0


def test_ops_quad_form_refuses_cpu_tensors():
    from gptq_gguf_toolkit_amd import _cabi, ops
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.quad_form(torch.zeros(4, 128), torch.zeros(128, 128))


# ------------------------------------------------------------------------------------------------ the fixture
def _fp64_H(xs):
    C = xs[0].shape[-1]
    H, n = torch.zeros(C, C, dtype=torch.float64), 0
    for x in xs:
        x2, b = x.reshape(-1, C).double(), x.shape[0]
        H = H * (n / (n + b)) + (2.0 / (n + b)) * (x2.T @ x2)
        n += b
    return H


def _fp64_quad(A, H, B=None):
    """The anchor of every test: ((D @ H~) * D).sum() in fp64, D formed by ONE subtraction in fp32 as the kernel does."""
    D = (A.float() - B.float()).double() if B is not None else A.double()
    H = H.double().clone()
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    return ((D @ H) * D).sum()


def test_fixture_fp64_expression_reproduces_the_reference():
    g = load_golden("G18_errest")
    xs = [torch.from_numpy(x).float() for x in g["inputs"]]
    W, H = torch.from_numpy(g["W"]), _fp64_H(xs)
    assert int((torch.diag(H) == 0).sum()) == 1 and float(H[int(g["dead"]), int(g["dead"])]) == 0.0
    # the reference's H after pre_step: fp32 of the same thing, the dead channel's diagonal entry set to 1
    Href = torch.from_numpy(g["H"]).double()
    assert float(Href[int(g["dead"]), int(g["dead"])]) == 1.0
    bound = 4 * float(g["rel_dist"].max())  # the reference's own fp32 distance (x 4: MKL builds differ in summation order)
    assert 0 < bound < 1e-5
    for w_c, want in zip(g["W_c"], g["errors"]):
        got = float(_fp64_quad(W, H, torch.from_numpy(w_c)) / _fp64_quad(W, H))
        rel = abs(got - float(want)) / abs(got)
        print(f"fixture: reference {want!r} fp64 {got!r} rel {rel:.3e} (bound {bound:.3e})")
        assert rel <= bound


# ------------------------------------------------------------------------------------------------ the driver
class _Counted(torch.Tensor):
    """What the stand-in's quad_form returns: a tensor that counts the host reads made through it or its results."""
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

    def __float__(self):
        _Counted.reads += 1
        return float(super().item())


def _fake_ops():
    me = types.SimpleNamespace(calls={"h_accumulate": 0, "quad_form": 0}, Hs=[])

    def h_accumulate(H, X, beta, alpha, ws=None):
        me.calls["h_accumulate"] += 1
        x = X.double()
        H.copy_((H.double() * beta + alpha * (x.T @ x)).float())
        return H

    def quad_form(A, H, B=None, ws=None):
        me.calls["quad_form"] += 1
        me.Hs.append(H)
        return _fp64_quad(A, H, B).as_subclass(_Counted)

    me.h_accumulate, me.quad_form = h_accumulate, quad_form
    return me


LEVELS = (("10-Q8.pth", 1e-3), ("4.5-Q4_K.pth", 2e-2), ("4-Q4_K.pth", 3e-2), ("3.pth", 1e-1))  # (file, sigma / rms(W))
ORDER = ["3.pth", "4-Q4_K.pth", "4.5-Q4_K.pth", "10-Q8.pth"]


@pytest.fixture()
def tiny(tmp_path, monkeypatch):
    from make_golden_shim import tiny_calib, tiny_llama
    import gptq_gguf_toolkit_amd.error_estimator as ee
    fake = _fake_ops()
    monkeypatch.setattr(ee, "_ops", fake)
    _Counted.reads = 0
    model = tiny_llama()
    g = torch.Generator().manual_seed(5)
    names = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and ".layers." in n]
    for n in names:
        W = model.get_submodule(n).weight.detach()
        os.makedirs(tmp_path / n)
        for f, s in LEVELS:
            torch.save(W + s * W.pow(2).mean().sqrt() * torch.randn(W.shape, generator=g), str(tmp_path / n / f))
        (tmp_path / n / "3-metadata.json").write_text(json.dumps({"tensor_info": {"name": n}}))  # not a level
    data = [([], {"input_ids": ids}) for ids in tiny_calib(n=3)]
    est = ee.ErrorEstimator(model, data, r".*layers.*((q|k|v|o|gate|up|down)_proj)$", ["model.embed_tokens"], "model.layers",
                            str(tmp_path), device="cpu")
    return ee, est, fake, model, names, data, tmp_path


def test_driver_shares_hessians_orders_levels_and_reads_once_per_linear(tiny, monkeypatch):
    ee, est, fake, model, names, data, db = tiny
    seen = {}
    inner = ee.ErrorEstimator._estimate_errors_group

    def spy(self, handles):
        for n, h in handles.items():
            seen[n] = h.hessian()
        return inner(self, handles)

    monkeypatch.setattr(ee.ErrorEstimator, "_estimate_errors_group", spy)
    # fp64 Hessians from hooks of the test's own (before the walk: it leaves the model as it was)
    acts, hooks = {}, []
    for n in names:
        hooks.append(model.get_submodule(n).register_forward_hook(
            lambda m, inp, out, n=n: acts.setdefault(n, []).append(inp[0].detach().clone())))
    with torch.no_grad():
        for _, kw in data:
            model(**kw)
    for h in hooks:
        h.remove()

    errors = est.estimate()
    assert list(errors) == [-1] and sorted(errors[-1]) == sorted(names) and len(names) == 14
    # q/k/v and gate/up share one Hessian OBJECT: 4 SYRKs per block and sample, not 7
    for b in range(2):
        p = f"model.layers.{b}."
        assert seen[p + "self_attn.q_proj"] is seen[p + "self_attn.k_proj"] is seen[p + "self_attn.v_proj"]
        assert seen[p + "mlp.gate_proj"] is seen[p + "mlp.up_proj"]
        assert len({id(seen[p + s]) for s in ("self_attn.q_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.down_proj")}) == 4
    assert est.hessians_built == 8 and fake.calls["h_accumulate"] == 2 * 4 * len(data)
    # the denominator once and one numerator per level; ONE host read per Linear
    assert fake.calls["quad_form"] == len(names) * (1 + len(LEVELS))
    assert _Counted.reads == len(names)
    # levels ordered by the float prefix, names kept next to the values; values are the fp64 expression
    for n in names:
        assert est.levels[n] == ORDER
        H = _fp64_H(acts[n])
        W = model.get_submodule(n).weight.detach()
        for f, got in zip(ORDER, errors[-1][n]):
            want = float(_fp64_quad(W, H, torch.load(str(db / n / f))) / _fp64_quad(W, H))
            assert abs(got - want) <= 1e-5 * want, (n, f, got, want)  # the stand-in keeps H in fp32
        assert errors[-1][n] == sorted(errors[-1][n], reverse=True)  # sigma falls as the level rises
    rep = ee.report(errors, est.levels)
    assert rep[names[0]] == [{"level": f[:-4], "error": e} for f, e in zip(ORDER, errors[-1][names[0]])]
    json.dumps(rep)
    assert set(est.estimate(group_by_numel=True)) == {256 * 256, 128 * 256, 512 * 256}


def test_level_key_is_the_float_prefix():
    from gptq_gguf_toolkit_amd.level_db import level_key
    assert level_key("4.5-Q4_K.pth") == 4.5 and level_key("4-Q4_K.pth") == 4.0 and level_key("3.pth") == 3.0
    assert level_key("10.pth") == 10.0 and level_key("2.5625-Q2_K.pth") == 2.5625
    with pytest.raises(ValueError):
        level_key("best.pth")


def test_conv_layers_and_other_modules_are_refused():
    from gptq_gguf_toolkit_amd.error_estimator import LayerErrorEstimator
    for layer in (torch.nn.Conv2d(4, 4, 3), torch.nn.Conv1d(4, 4, 1), torch.nn.Embedding(8, 8)):
        with pytest.raises(TypeError, match="nn.Linear only"):
            LayerErrorEstimator(layer)
    LayerErrorEstimator(torch.nn.Linear(128, 8))


def test_more_than_one_rank_is_refused(tiny, monkeypatch):
    ee, est, fake, *_ = tiny
    monkeypatch.setattr(ee.dist_utils, "is_dist_available_and_initialized", lambda: True)
    monkeypatch.setattr(ee.dist_utils, "get_world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="one rank"):
        est.estimate()
    assert fake.calls["h_accumulate"] == 0
    h = ee.LayerErrorEstimator(torch.nn.Linear(128, 8))
    h.update(torch.randn(1, 4, 128))
    with pytest.raises(NotImplementedError, match="one rank"):
        h.pre_step()


def test_layer_estimator_surface(tiny):
    ee, *_ = tiny
    g = load_golden("G18_errest")
    layer = torch.nn.Linear(256, 48)
    layer.weight.data = torch.from_numpy(g["W"])
    h = ee.LayerErrorEstimator(layer)
    with pytest.raises(AssertionError):
        h.pre_step()  # no sample yet
    for x in g["inputs"]:
        h.update(torch.from_numpy(x).float())
    assert h.num_samples == 2
    with pytest.raises(AssertionError):
        h.estimate(layer.weight)  # pre_step first
    h.pre_step()
    H0 = h.H.clone()
    vals = [h.estimate(torch.from_numpy(w)) for w in g["W_c"]]
    assert all(v.dtype == torch.float64 and v.dim() == 0 for v in vals)
    assert torch.equal(h.H, H0) and float(h.H[int(g["dead"]), int(g["dead"])]) == 0.0  # H is the caller's: not written
    bound = 4 * float(g["rel_dist"].max()) + 1e-6  # + the stand-in's fp32 H
    for v, want in zip(vals, g["errors"]):
        assert abs(float(v) - float(want)) <= bound * float(want)
    with pytest.raises(ValueError, match="shape"):
        h.estimate(torch.zeros(48, 128))
    h.reset()
    assert h.H is None and h.num_samples == 0 and not h.pre_step_completed


# ------------------------------------------------------------------------------------------------ the CLI
def test_cli_arguments(tmp_path, capsys):
    from gptq_gguf_toolkit_amd.error_estimator import parse_args
    calib, db = tmp_path / "calib.pt", tmp_path / "db"
    torch.save([torch.zeros(1, 8, dtype=torch.long)], str(calib))
    db.mkdir()
    base = ["--model_name_or_path", "m", "--calibration_data", str(calib), "--quant_weights_path", str(db),
            "--output_file", str(tmp_path / "o.json")]
    a = parse_args(base)
    assert a.dtype == "float16" and a.calibration_tokens is None and a.sequence_length is None and not a.verbose
    a = parse_args(base + ["--calibration_tokens", "4096", "--sequence_length", "512", "--dtype", "bfloat16", "--verbose"])
    assert (a.calibration_tokens, a.sequence_length, a.dtype, a.verbose) == (4096, 512, "bfloat16", True)
    for bad in (["--calibration_data", "wikitext2"], ["--quant_weights_path", str(tmp_path / "nope")], ["--dtype", "int8"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    assert "downloads are not part" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(base[2:])  # --model_name_or_path is required
