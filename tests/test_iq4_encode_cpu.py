"""The IQ4_NL / IQ4_XS encoder, host side (no GPU): the additive header include/gptq_gguf_iq4_encode.h and its binding, the
refusals of gq_quantize_iq4 -- made before the first HIP call, so host pointers do --, the options' rules, and the host form
gguf_writer.quantize_iq4 against the element-by-element restatement of the contract (tests/iq4_encode_spec.py), byte for byte."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import iq4_encode_spec as S  # noqa: E402
import iq4_spec  # noqa: E402

NL, XS = S.NL, S.XS
P = 256  # any 16-byte aligned address, never dereferenced


def _msg(L):
    return L.gq_last_error().decode()


def host(x, t, imp=None):
    from gptq_gguf_toolkit_amd.gguf_writer import quantize_iq4
    return quantize_iq4(x, t, imp)


def test_header_symbol_is_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_iq4_encode.h")).read()
    declared = set(re.findall(r"^int (gq_[a-z0-9_]+)\s*\(", hdr, re.M))
    L = _cabi.lib()
    assert declared == set(_cabi.EXPORTS_IQ4_ENCODE) == {"gq_quantize_iq4"}
    assert hasattr(ctypes.CDLL(_cabi.SO_PATH), "gq_quantize_iq4") and len(L.gq_quantize_iq4.argtypes) == 9
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6  # additive: the version stays
    # the header says whose contract this is, and what is outside it
    assert "ntry = 7" in hdr and "quantize_row_iq4_nl_impl" in hdr and "llama.cpp build" in hdr and "Non-finite" in hdr
    assert "gptq_gguf_iq4_encode.h" in open(os.path.join(ROOT, "include", "gptq_gguf_iq4.h")).read()
    assert "gptq_gguf_iq4_encode.h" in open(os.path.join(ROOT, "README.md")).read()
    assert "`gq_quantize_iq4`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_argument_checks_need_no_device():
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()
    q = L.gq_quantize_iq4
    assert q(P, 0, 4, 288, XS, None, None, P, None) == -2 and "C=288" in _msg(L)      # IQ4_XS: C % 256
    assert q(P, 0, 4, 40, NL, None, None, P, None) == -2 and "C=40" in _msg(L)        # IQ4_NL: C % 32
    assert q(P, 0, 0, 256, XS, None, None, P, None) == -2 and "R=0" in _msg(L)
    assert q(P, 0, 4, 1 << 31, NL, None, None, P, None) == -2
    assert q(P, 7, 4, 256, XS, None, None, P, None) == -1 and "x_dtype 7" in _msg(L)
    for t in (8, 12, 21, 22):
        assert q(P, 0, 4, 256, t, None, None, P, None) == -1 and f"q_type {t}" in _msg(L)
    assert q(None, 0, 4, 256, XS, None, None, P, None) == -6 and q(P, 1, 4, 256, NL, None, None, None, None) == -6
    assert q(P + 8, 2, 4, 256, XS, None, None, P, None) == -2 and "16-byte aligned" in _msg(L)
    assert q(P, 2, 4, 256, XS, None, None, P + 8, None) == -2 and "16-byte aligned" in _msg(L)
    assert q(P, 2, 4, 256, XS, P + 4, None, P, None) == -2 and "importance" in _msg(L)
    assert q(P, 2, 4, 256, XS, None, P + 2, P, None) == -2 and "row_src" in _msg(L)
    assert L.gq_quantize_q8_0(P, 0, 4, 64, None, P + 2, None) == -2  # (the neighbour's checks are its own)


def test_ops_refusals_come_before_any_device_work():
    from gptq_gguf_toolkit_amd import _cabi, ops
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.quantize_iq4(torch.zeros(4, 256), XS)


def test_options_need_a_level_db(monkeypatch, capsys, tmp_path):
    from gptq_gguf_toolkit_amd.quant import levels_problem, parse_args
    from gptq_gguf_toolkit_amd.quantizer import Quantizer
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    model = tmp_path / "model"
    model.mkdir()
    base = ["--model_name_or_path", str(model), "--quantizable_modules", "x", "--pre_block_modules", "e", "--block_modules", "b",
            "--calibration_data", "c.pt", "--save_dir", "s"]
    lv = ["--levels", "Q2_K", "Q4_K", "--propagate_level", "Q4_K"]
    for extra in (["--level_db_iq4", "IQ4_XS"], lv + ["--level_db_iq4", "IQ4_XS", "IQ4_NL"]):
        with pytest.raises(SystemExit) as e:
            parse_args(base + extra)
        assert e.value.code == 2 and "--level_db_iq4 needs --level_db" in capsys.readouterr().err
    a = parse_args(base + lv + ["--level_db", str(tmp_path / "db"), "--level_db_iq4", "IQ4_XS", "IQ4_NL"])
    assert a.level_db_iq4 == ["IQ4_XS", "IQ4_NL"] and a.level_db_iq4_importance == "hessian" and levels_problem(a) is None
    a = parse_args(base + lv + ["--level_db", str(tmp_path / "db"), "--level_db_iq4", "IQ4_NL", "--level_db_iq4_importance", "none"])
    assert a.level_db_iq4 == ["IQ4_NL"] and a.level_db_iq4_importance == "none"
    assert parse_args(base + lv + ["--level_db", str(tmp_path / "db")]).level_db_iq4 == []
    with pytest.raises(SystemExit):
        parse_args(base + lv + ["--level_db", str(tmp_path / "db"), "--level_db_iq4", "IQ3_S"])
    assert "invalid choice" in capsys.readouterr().err
    ns = types.SimpleNamespace(levels=None, propagate_level=None, level_db=None, level_db_only=False, level_db_q8_0=False,
                               level_db_iq4=["IQ4_XS"])
    assert "--level_db_iq4 needs --level_db" in levels_problem(ns)
    drv = Quantizer.__new__(Quantizer)
    drv.quantizer_kwargs = {}
    with pytest.raises(ValueError, match="level_db_iq4 needs level_db"):
        drv.quantize_levels([10, 12], 12, level_db=None, level_db_iq4=("IQ4_XS",))


# ------------------------------------------------------------------------------------------------ host form == loop spec
@pytest.mark.parametrize("t,R,C", [(XS, 5, 512), (NL, 5, 96)])
@pytest.mark.parametrize("weighted", [False, True])
def test_host_form_equals_the_loop_spec_on_random_data(t, R, C, weighted):
    x = S.random_matrix(R, C, seed=t + R)
    imp = S.random_importance(C, seed=t) if weighted else None
    got = host(x, t, imp)
    bs, ts = S.GEOMETRY[t]
    assert got.dtype == np.uint8 and got.shape == (R, C // bs * ts)
    assert got.tobytes() == S.encode(t, x, imp).tobytes()
    y = iq4_spec.decode(t, got)
    assert np.isfinite(y).all()
    rel = float(np.sqrt(((y - x) ** 2).sum() / (x ** 2).sum()))
    print(f"    {S.GEOMETRY[t]} weighted={weighted}: relative rms round trip {rel:.4f}")
    assert rel < 0.12  # a 4-bit code of Gaussian data: 7 .. 8 % (this is a sanity bound, not the claim)
    if t == XS:
        ls = S.xs_scales(got)
        assert ls.min() >= 0 and ls.max() <= 63


@pytest.mark.parametrize("t", [XS, NL])
@pytest.mark.parametrize("weighted", [False, True])
def test_host_form_equals_the_loop_spec_on_the_crafted_blocks(t, weighted):
    x, imp = S.crafted(t)
    imp = imp if weighted else None
    got = host(x, t, imp)
    assert got.tobytes() == S.encode(t, x, imp).tobytes()
    bs, ts = S.GEOMETRY[t]
    b = got.reshape(x.shape[0], -1, ts)
    qs = b[:, :, ts - bs // 2:]
    y = iq4_spec.decode(t, got)
    assert np.isfinite(y).all()
    # rows 0 (all zero) and 1 (amax = 1e-20): d = 0, code 8 everywhere
    for r in (0, 1):
        assert (qs[r] == 0x88).all() and not b[r, :, :2].copy().view(np.float16).astype(np.float32).any() and not y[r].any()
    if t == XS:
        ls = S.xs_scales(got).reshape(x.shape[0], -1, 8)
        assert ls.min() >= 0 and ls.max() <= 63
        assert (ls[:2] == 32).all()
        # row 4, super-block 0: block 2 is 100 x the others -> l = -32 for it, l = 0 (code 8 everywhere) for the others
        assert ls[4, 0].tolist() == [32, 32, 0, 32, 32, 32, 32, 32]
        assert (qs[4, 0, :32] == 0x88).all() and (qs[4, 0, 48:] == 0x88).all() and not (qs[4, 0, 32:48] == 0x88).all()
    # rows 2 / 3: +m and -m tied for amax -- `max` is the first one, and the two orders give different blocks
    assert b[2, 0].tobytes() != b[3, 0].tobytes()
    # row 6: products that land exactly on table entries and on midpoints between them did occur in the search (itry = 0)
    step = np.float32(2.0 ** -12)
    a = x[6, :32] * (np.float32(1) / step)
    assert set(a[:16].tolist()) == set(float(v) for v in S.KV)
    assert [S.best(v) for v in a[:16]] == list(range(16))
    assert [S.best(v) for v in a[16:31]] == list(range(1, 16))  # a tie goes up


def test_best_compares_rounded_differences_not_a_midpoint():
    """best() at the edges of the table, on entries, and around the midpoints -4.5 of (-10, 1) and 101 of (89, 113): a tie goes
    up, one ulp below a midpoint goes down.  The host form's vectorised best() agrees with the scalar one."""
    from gptq_gguf_toolkit_amd.gguf_writer import _iq4_best
    a = np.nextafter(np.float32(-4.5), np.float32(-10))   # just below the midpoint of (-10, 1)
    assert S.best(a) == int(_iq4_best(np.array([a], np.float32))[0]) == 7
    assert S.best(np.float32(-4.5)) == int(_iq4_best(np.array([-4.5], np.float32))[0]) == 8  # the tie goes up
    for v in (-1000.0, -127.0, -126.9, 0.0, 112.9, 113.0, 5000.0):
        assert S.best(np.float32(v)) == int(_iq4_best(np.array([v], np.float32))[0])
    assert S.best(np.float32(0)) == 8
    # between 89 and 113 (midpoint 101): 101 + 2^-18 is representable, and (a - 89) rounds to 12 + 2^-18 exactly while
    # (113 - a) = 12 - 2^-18: up.  One ulp below the midpoint goes down.
    assert S.best(np.nextafter(np.float32(101), np.float32(200))) == 15 and S.best(np.nextafter(np.float32(101), np.float32(0))) == 14


# ------------------------------------------------------------------------------------------------ the encoder is honest
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_the_search_beats_the_naive_code_and_importance_lowers_the_weighted_error(seed):
    x, qw = S.honest_case(seed)
    kv = np.array(S.KV, np.float32)
    # (a) unweighted IQ4_NL against d = max / kv[0] with the nearest entry
    y = iq4_spec.decode(NL, host(x, NL))
    xb = x.reshape(-1, 32)
    mx = xb[np.arange(len(xb)), np.abs(xb).argmax(axis=1)]
    d = (mx / kv[0]).astype(np.float32)
    near = kv[np.abs(xb[:, :, None] / d[:, None, None] - kv[None, None, :]).argmin(axis=2)] * d[:, None]
    e_search, e_naive = float(((y - x) ** 2).sum()), float(((near.reshape(x.shape) - x) ** 2).sum())
    print(f"    seed {seed}: (a) search / naive = {e_search / e_naive:.4f}")
    assert e_search < e_naive
    # (b) the weighted error with importance = qw against the same without
    for t in (XS, NL):
        e_w = float((qw * (iq4_spec.decode(t, host(x, t, qw)) - x) ** 2).sum())
        e_u = float((qw * (iq4_spec.decode(t, host(x, t)) - x) ** 2).sum())
        print(f"    seed {seed}: (b) {iq4_spec.NAME[t]} weighted / unweighted = {e_w / e_u:.4f}")
        assert e_w < e_u
