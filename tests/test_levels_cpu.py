"""The one-pass level build, host side on the CPU: the pure band layout, the CLI's refusals, the tree naming, the
header / binding constant, and the driver's level mode (Quantizer.quantize_levels -> BlockSchedule.quantize_levels ->
GPTQ.compute_levels) with the compute backend replaced by tests/fake_ops.py plus an oracle-backed band walk."""
import os
import re
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

Q2, Q3, Q4, Q5, Q6 = 10, 11, 12, 13, 14


def test_band_layout_row_ends_and_sm_offsets():
    from gptq_gguf_toolkit_amd.ops import BANDS_MAX, band_layout
    C = 512
    # G = 32 (Q4_K), 16 (Q6_K), 16 (Q2_K), 32 (Q5_K), 16 (Q3_K): uneven rows, mixed group sizes
    lay, total = band_layout([(128, Q4), (192, Q6), (384, Q2), (448, Q5), (512, Q3)], C)
    assert [(r0, r1) for r0, r1, *_ in lay] == [(0, 128), (128, 192), (192, 384), (384, 448), (448, 512)]
    assert [g for *_, g, _ in lay] == [32, 16, 16, 32, 16]
    want = [0, 128 * 16, 128 * 16 + 64 * 32, 128 * 16 + 64 * 32 + 192 * 32, 128 * 16 + 64 * 32 + 192 * 32 + 64 * 16]
    assert [off for *_, off in lay] == want
    assert total == want[-1] + 64 * 32 and total <= 512 * (C // 16)
    one, tot1 = band_layout([(64, Q4)], 256)
    assert one == [(0, 64, Q4, 32, 0)] and tot1 == 64 * 8
    for bad in ([(128, Q4), (64, Q2)], [(64, Q4), (64, Q2)], [(96, Q4)], [(64, 9)], [],
                [(64 * (k + 1), Q4) for k in range(BANDS_MAX + 1)]):
        with pytest.raises(ValueError):
            band_layout(bad, C)
    assert len(band_layout([(64 * (k + 1), Q4) for k in range(BANDS_MAX)], C)[0]) == BANDS_MAX


def test_header_constant_equals_the_binding():
    from gptq_gguf_toolkit_amd import _cabi, ops
    text = open(os.path.join(ROOT, "include", "gptq_gguf_levels.h")).read()
    m = re.search(r"#define\s+GQ_BANDS_MAX\s+(\d+)", text)
    assert m and int(m.group(1)) == _cabi.BANDS_MAX == ops.BANDS_MAX
    assert "gq_gptq_quantize_bands" in _cabi.EXPORTS_LEVELS and "gq_gptq_quantize_bands(" in text
    import ctypes
    assert ctypes.sizeof(_cabi.Band) == 16  # int64 row_end, int32 q_type, padded as the C struct is


BASE = ["--model_name_or_path", "m", "--quantizable_modules", "x", "--pre_block_modules", "e", "--block_modules", "b",
        "--calibration_data", "c.pt", "--save_dir", "s"]


def test_cli_level_flags(monkeypatch, capsys, tmp_path):
    from gptq_gguf_toolkit_amd.quant import levels_problem, parse_args
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = parse_args(BASE + ["--levels", "Q2_K", "Q4_K", "Q6_K", "--propagate_level", "Q4_K"])
    assert a.levels == ["Q2_K", "Q4_K", "Q6_K"] and a.propagate_level == "Q4_K"
    a = parse_args(BASE + ["--levels", "Q2_K", "Q3_K", "Q4_K", "Q5_K", "Q6_K", "--propagate_level", "none"])
    assert a.propagate_level == "none" and levels_problem(a) is None
    a = parse_args(BASE)  # an ordinary run knows nothing of levels
    assert a.levels is None and a.propagate_level is None
    cfg = tmp_path / "bits.json"
    cfg.write_text("{}")
    refused = {
        "needs --propagate_level": ["--levels", "Q2_K", "Q4_K"],
        "needs --levels": ["--propagate_level", "Q4_K"],
        "not one of --levels": ["--levels", "Q2_K", "Q4_K", "--propagate_level", "Q6_K"],
        "twice": ["--levels", "Q4_K", "Q4_K", "--propagate_level", "Q4_K"],
        "--bit_width_configuration": ["--levels", "Q4_K", "--propagate_level", "Q4_K", "--bit_width_configuration", str(cfg)],
        "--act_order": ["--levels", "Q4_K", "--propagate_level", "Q4_K", "--act_order", "--static_groups"],
        "--static_groups": ["--levels", "Q4_K", "--propagate_level", "none", "--static_groups"],
        "invalid choice": ["--levels", "Q8_0", "--propagate_level", "none"],
    }
    for msg, extra in refused.items():
        with pytest.raises(SystemExit) as e:
            parse_args(BASE + extra)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err, msg
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        parse_args(BASE + ["--levels", "Q4_K", "--propagate_level", "Q4_K"])
    assert "one rank" in capsys.readouterr().err
    parse_args(BASE)  # two ranks without --levels: as before


def test_run_quant_sh_passes_the_flags_through():
    text = open(os.path.join(ROOT, "gptq-gguf-toolkit_amd", "run_quant.sh")).read()
    assert "${LEVELS:+--levels $LEVELS}" in text and '${PROPAGATE_LEVEL:+--propagate_level "$PROPAGATE_LEVEL"}' in text


def test_tree_naming_and_level_checks():
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    from gptq_gguf_toolkit_amd.quantizer import check_levels, level_tree_name
    assert level_tree_name(T.Q4_K, "model.layers.0.mlp.up_proj") == "Q4_K/model.layers.0.mlp.up_proj"
    assert level_tree_name(14, "lm_head") == "Q6_K/lm_head"
    assert check_levels([10, 12], 12) == ([T.Q2_K, T.Q4_K], T.Q4_K) and check_levels([T.Q3_K], None) == ([T.Q3_K], None)
    for lv, pr in (([], None), ([12, 12], None), ([10, 12], 14), ([9], None)):
        with pytest.raises(ValueError):
            check_levels(lv, pr)


# ---- the driver's level mode on the CPU backend -------------------------------------------------------------------
def _fake_bands(fake):
    """gptq_quantize_bands for tests/fake_ops.py: the oracle, band by band -- what the contract of the HIP entry point says."""
    calls = {"n": 0, "bands": []}

    def gptq_quantize_bands(W, U, bands, block_size=128, rmin=-1.0, rdelta=0.1, nstep=20, ws=None, **mq):
        from gptq_gguf_toolkit_amd.ops import band_layout
        lay, _ = band_layout(bands, W.shape[1])
        assert lay[-1][1] == W.shape[0]
        calls["n"] += 1
        calls["bands"].append(len(bands))
        out = []
        for r0, r1, t, _, _ in lay:
            out.append(fake.gptq_quantize(W[r0:r1], U, t, block_size, False, rmin, rdelta, nstep, **mq))
            fake.calls["gptq_quantize"] -= 1
        return out
    return gptq_quantize_bands, calls


def _driver(save_dir, non_block=False):
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd.quantizer import Quantizer
    data = [([], {"input_ids": ids}) for ids in tiny_calib()]
    model = tiny_llama()
    return model, Quantizer(model, data_loader=data, quantizable_modules=r".*layers.*((q|k|v|o|gate|up|down)_proj)$",
                            quantizer_kwargs=dict(rel_damp=0.01, block_size=128, act_order=False, quant_scale="absmax",
                                                  static_groups=False, rmin=-1.0, rdelta=0.1, nstep=20, verbose=False),
                            pre_block_modules=["model.embed_tokens"], block_modules="model.layers",
                            post_block_modules=["lm_head"], quant_non_block_modules=non_block, device="cpu",
                            save_dir=str(save_dir))


def _same_tree(a, b, only=None):
    names = sorted(n for n in os.listdir(a) if only is None or only in n)
    assert names == sorted(n for n in os.listdir(b) if only is None or only in n) and names
    for n in names:
        x = torch.load(os.path.join(a, n, "data.pth"), weights_only=True)
        y = torch.load(os.path.join(b, n, "data.pth"), weights_only=True)
        assert set(x) == set(y)
        for k in x:
            assert (x[k] == y[k]) if k == "q_type" else (x[k].dtype == y[k].dtype and torch.equal(x[k], y[k])), (n, k)


def test_driver_level_mode_equals_the_ordinary_runs(tmp_path, monkeypatch):
    """quantize_levels([Q2_K, Q4_K, Q6_K], propagate=Q4_K) with embed / lm_head: the Q4_K tree and the model equal an
    ordinary all-Q4_K run; block 0 and the non-block modules of the other trees equal their ordinary runs; one band walk
    per chain (4 per block) and no more factorisations than a single-level run.  propagate=None: the model is untouched."""
    import fake_ops
    from gptq_gguf_toolkit_amd.quant import DEFAULT_KEYS
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    fake = fake_ops.install(monkeypatch)
    bands_fn, calls = _fake_bands(fake)
    monkeypatch.setattr(fake, "gptq_quantize_bands", bands_fn, raising=False)
    monkeypatch.setattr(fake, "BANDS_MAX", 64, raising=False)
    levels = [T.Q2_K, T.Q4_K, T.Q6_K]
    model, drv = _driver(tmp_path / "lv", non_block=True)
    drv.quantize_levels(levels, T.Q4_K)
    lv_stats, lv_prepares = dict(drv.schedule_stats), fake.calls["h_prepare"]
    assert sorted(os.listdir(tmp_path / "lv")) == ["Q2_K", "Q4_K", "Q6_K"]
    assert calls["n"] == 2 * 4 and fake.calls["gptq_quantize"] == 0  # one walk per chain: qkv, o, gate/up, down
    assert sorted(calls["bands"]) == sorted(2 * [9, 3, 6, 3])
    ordinary = {}
    for t in levels:
        for k in fake.calls:
            fake.calls[k] = 0
        m, d = _driver(tmp_path / t.name, non_block=True)
        d.quantize({k: t for k in DEFAULT_KEYS})
        ordinary[t] = (m, dict(d.schedule_stats), fake.calls["h_prepare"])
    _same_tree(tmp_path / "lv" / "Q4_K", tmp_path / "Q4_K")
    for (n, p), (n2, p2) in zip(sorted(model.named_parameters()), sorted(ordinary[T.Q4_K][0].named_parameters())):
        assert n == n2 and torch.equal(p, p2), n
    for t in (T.Q2_K, T.Q6_K):
        _same_tree(tmp_path / "lv" / t.name, tmp_path / t.name, only=".layers.0.")
        _same_tree(tmp_path / "lv" / t.name, tmp_path / t.name, only="embed_tokens")
        _same_tree(tmp_path / "lv" / t.name, tmp_path / t.name, only="lm_head")
    assert lv_stats["own_U"] <= ordinary[T.Q4_K][1]["own_U"] and lv_prepares <= ordinary[T.Q4_K][2]
    assert lv_stats["syrk_launches"] == ordinary[T.Q4_K][1]["syrk_launches"]

    model0, drv0 = _driver(tmp_path / "none")
    before = {n: p.detach().clone() for n, p in model0.named_parameters()}
    drv0.quantize_levels(levels, None)
    for n, p in model0.named_parameters():
        assert torch.equal(p, before[n]), n
    for t in levels:
        _same_tree(tmp_path / "none" / t.name, tmp_path / t.name, only=".layers.0.")


def test_compute_levels_cuts_long_band_lists_and_walks_odd_rows_alone(monkeypatch):
    """More than GQ_BANDS_MAX bands are cut into several calls; a handle whose rows are no multiple of 64 walks its levels
    one after another with the shared U; act_order / static_groups are refused.  Every result equals quantize(t) of a
    fresh handle."""
    import fake_ops
    from gptq_gguf_toolkit_amd.gptq import GPTQ
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    fake = fake_ops.install(monkeypatch)
    bands_fn, calls = _fake_bands(fake)
    monkeypatch.setattr(fake, "gptq_quantize_bands", bands_fn, raising=False)
    monkeypatch.setattr(fake, "BANDS_MAX", 4, raising=False)  # two levels: two handles to a call
    torch.manual_seed(3)
    rows, C = [64, 64, 40, 64], 256
    lins = [torch.nn.Linear(C, r, bias=False) for r in rows]
    xs = [torch.randn(1, 80, C) * torch.exp(torch.randn(C) * 0.3) for _ in range(2)]
    kw = dict(rel_damp=0.01, block_size=128)

    def handles():
        hs = [GPTQ(l, **kw) for l in lins]
        for h in hs[1:]:
            h.shared_H_with, hs[0]._has_followers = hs[0], True
        for x in xs:
            for h in hs:
                h.update(x)
        for h in hs:
            h.quantization_pre_step()
        return hs

    levels = [T.Q3_K, T.Q5_K]
    hs = handles()
    got = GPTQ.compute_levels(hs, levels)
    assert calls["bands"] == [4, 2] and all(h.W is None for h in hs)  # (64, 64) then (64); the 40-row handle alone
    for i, l in enumerate(lins):
        for t in levels:
            f = GPTQ(l, **kw)
            for x in xs:
                f.update(x)
            want = f.quantize(t)
            for a, b in zip(got[hs[i]][t], want):
                assert a.dtype == b.dtype and torch.equal(a, b), (i, t)
    for bad in (dict(act_order=True, static_groups=True), dict(static_groups=True)):
        with pytest.raises(ValueError):
            GPTQ.compute_levels([GPTQ(lins[0], **kw, **bad)], levels)
    with pytest.raises(ValueError):
        GPTQ.compute_levels(handles()[:1], [T.Q4_K, T.Q4_K])
