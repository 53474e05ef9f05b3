"""GPTQ's column walk on the IQ4_XS / IQ4_NL grid, host side (no GPU): the additive header include/gptq_gguf_iq4_gptq.h and its
binding, the refusals of gq_gptq_quantize_iq4 / gq_pack_iq4 -- made before the first HIP call, so host pointers do --, and
the properties of the contract on its loop restatement tests/iq4_gptq_spec.py: with U = I the bytes of the RTN encoder, W equal
to the decode of its own bytes, and the quality condition on the two correlated problems."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import iq4_encode_spec as ES  # noqa: E402
import iq4_gptq_spec as S  # noqa: E402
import iq4_spec  # noqa: E402

NL, XS = S.NL, S.XS
P = 256  # any 16-byte aligned address, never dereferenced


def _msg(L):
    return L.gq_last_error().decode()


def host(x, t, imp=None):
    from gptq_gguf_toolkit_amd.gguf_writer import quantize_iq4
    return quantize_iq4(x, t, imp)


def test_header_symbols_are_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_iq4_gptq.h")).read()
    declared = set(re.findall(r"^int (gq_[a-z0-9_]+)\s*\(", hdr, re.M))
    L = _cabi.lib()
    assert declared == set(_cabi.EXPORTS_IQ4_GPTQ) == {"gq_gptq_quantize_iq4", "gq_pack_iq4"}
    so = ctypes.CDLL(_cabi.SO_PATH)
    assert hasattr(so, "gq_gptq_quantize_iq4") and len(L.gq_gptq_quantize_iq4.argtypes) == 15
    assert hasattr(so, "gq_pack_iq4") and len(L.gq_pack_iq4.argtypes) == 9
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6  # additive: the version stays
    assert "11 + 5 + 7" in hdr and "a tie goes up" in hdr and "correctly rounded" in hdr


def test_argument_checks_need_no_device():
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()
    need = L.gq_workspace_bytes(_cabi.WS_GPTQ_QUANTIZE, 64, 256, 0, 128)

    def walk(W=P, U=P, R=64, C=256, t=XS, block=128, imp=None, q=P, d=P, ls=P, step=P, istep=P, ws=P, nws=need):
        return L.gq_gptq_quantize_iq4(W, U, R, C, t, block, imp, q, d, ls, step, istep, ws, nws, None)
    for t in (8, 12, 21, 22):
        assert walk(t=t) == -1 and f"q_type {t}" in _msg(L)
    for t in (XS, NL):  # the walk's rule for both types
        assert walk(t=t, C=288) == -2 and "C=288" in _msg(L)
        assert walk(t=t, C=32) == -2
    assert walk(R=0) == -2
    for name in ("W", "U", "q", "d", "step", "istep"):
        assert walk(**{name: None}) == -6, name
    assert walk(ls=None) == -6 and walk(t=NL, ls=None, nws=0) == -3  # IQ4_NL needs no ls: the next check speaks
    assert walk(imp=P + 4) == -2 and "importance" in _msg(L)
    assert walk(block=24) == -4 and "multiple of 16" in _msg(L)
    assert walk(nws=need - 1) == -3 and walk(ws=None) == -3

    def pack(t=XS, R=4, C=256, q=P, d=P, ls=P, rs=None, out=P):
        return L.gq_pack_iq4(t, R, C, q, d, ls, rs, out, None)
    for t in (8, 12, 21, 22):
        assert pack(t=t) == -1 and f"q_type {t}" in _msg(L)
    assert pack(C=288) == -2 and pack(t=NL, C=40) == -2 and pack(R=0) == -2
    assert pack(q=None) == -6 and pack(d=None) == -6 and pack(out=None) == -6 and pack(ls=None) == -6
    assert pack(q=P + 8) == -2 and pack(out=P + 8) == -2 and "16-byte aligned" in _msg(L)
    assert pack(rs=P + 2) == -2 and "row_src" in _msg(L)


def test_ops_refuse_host_tensors():
    from gptq_gguf_toolkit_amd import _cabi, ops
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.gptq_quantize_iq4(torch.zeros(4, 256), torch.eye(256), XS)
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.pack_iq4(XS, torch.zeros(4, 256, dtype=torch.uint8), torch.zeros(4, 1, dtype=torch.float16),
                     torch.zeros(4, 8, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------------------- the spec
def test_best_on_a_vector_is_the_loop_best():
    rng = np.random.default_rng(0)
    k = np.array(ES.KV, np.float32)
    a = np.concatenate([rng.uniform(-140, 130, 4000), k, (k[:-1] + k[1:]) / 2, [-1e30, 1e30, 0.0, -0.0]]).astype(np.float32)
    assert np.array_equal(S.best_fast(a), S.best(a))


@pytest.mark.parametrize("t", [XS, NL])
def test_both_scale_searches_agree(t):
    x, imp = ES.crafted(t)
    if t == NL:  # one 256-column panel of crafted NL rows
        x, imp = np.tile(x, (1, 4)), np.tile(imp, 4)
    else:
        x, imp = x[:, :256], imp[:256]
    for im in (None, imp):
        for a, b in zip(S.loop_scales(t, x, im), S.host_scales(t, x, im)):
            assert (a is None and b is None) or np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b, a.dtype).view(np.uint8))


def test_the_walk_is_the_same_under_the_loop_forms():
    """The whole walk with the element-by-element scale search and best() equals the walk with the vectorised ones."""
    W, H, diag = S.correlated_problem(np.random.default_rng(5), 3, 256, 16, 0.3)
    U = S.upper_factor(H)
    for t in (XS, NL):
        a = S.walk(W, U, t, 128, diag, scales=S.loop_scales, best=S.best)
        b = S.walk(W, U, t, 128, diag)
        for n in a:
            assert (a[n] is None and b[n] is None) or np.array_equal(a[n].view(np.uint8), b[n].view(np.uint8)), (t, n)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("t", [XS, NL])
def test_with_the_identity_the_walk_is_the_rtn_encoder(t, weighted):
    W = ES.random_matrix(6, 512, 3)
    W[2, 256:] = 0      # an all-zero super-block
    W[3, 32:64] = 0     # an all-zero block in a live one
    imp = ES.random_importance(512, 3) if weighted else None
    if weighted:
        imp[64:96] = 0  # all zero over one block
    out = S.walk(W, np.eye(512, dtype=np.float32), t, 128, imp)
    assert np.array_equal(S.pack(t, out), host(W, t, imp))


@pytest.mark.parametrize("block", [128, 192])
@pytest.mark.parametrize("t", [XS, NL])
def test_the_walks_w_is_the_decode_of_its_bytes(t, block):
    W, H, diag = S.correlated_problem(np.random.default_rng(7), 5, 512, 32, 0.3)
    out = S.walk(W, S.upper_factor(H), t, block, diag)
    dec = iq4_spec.decode(t, S.pack(t, out))
    assert not np.isnan(out["W"]).any() and np.array_equal(out["W"], dec)  # (== on values: the sign of a zero is not compared)
    assert not np.array_equal(S.pack(t, out), host(W, t, diag))  # the error feedback moved something


def test_quality_on_the_correlated_problems():
    """sum(dW H o dW) / sum(W H o W) of the walk against round-to-nearest with the same importance: below half of it.  (An
    fp64 prototype of the walk stood at 0.15 and 0.07 of RTN's error on these two problems.)"""
    for W, H, diag in S.quality_problems():
        out = S.walk(W, S.upper_factor(H), XS, 128, diag)
        rtn = iq4_spec.decode(XS, host(W, XS, diag))
        e_gptq, e_rtn = S.relative_error(W, out["W"], H), S.relative_error(W, rtn, H)
        print(f"[{W.shape[0]} x {W.shape[1]}] RTN {e_rtn:.3e}  GPTQ {e_gptq:.3e}  ratio {e_gptq / e_rtn:.3f}")
        assert e_gptq < 0.5 * e_rtn


# ------------------------------------------------------------------------------------------------------------- the option
def test_the_method_needs_an_iq4_level_and_a_known_name(monkeypatch, capsys, tmp_path):
    from gptq_gguf_toolkit_amd.quant import levels_problem, parse_args
    from gptq_gguf_toolkit_amd.quantizer import check_iq4_levels
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    model = tmp_path / "model"
    model.mkdir()
    base = ["--model_name_or_path", str(model), "--quantizable_modules", "x", "--pre_block_modules", "e", "--block_modules", "b",
            "--calibration_data", "c.pt", "--save_dir", "s", "--levels", "Q2_K", "Q4_K", "--propagate_level", "Q4_K",
            "--level_db", str(tmp_path / "db")]
    with pytest.raises(SystemExit) as e:
        parse_args(base + ["--level_db_iq4_method", "gptq"])
    assert e.value.code == 2 and "--level_db_iq4_method needs --level_db_iq4" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(base + ["--level_db_iq4", "IQ4_XS", "--level_db_iq4_method", "obq"])
    capsys.readouterr()
    a = parse_args(base + ["--level_db_iq4", "IQ4_XS"])
    assert a.level_db_iq4_method == "rtn" and levels_problem(a) is None  # the default changes nothing
    a = parse_args(base + ["--level_db_iq4", "IQ4_XS", "IQ4_NL", "--level_db_iq4_method", "gptq"])
    assert a.level_db_iq4_method == "gptq" and levels_problem(a) is None
    assert check_iq4_levels(("IQ4_XS", "IQ4_NL"), "hessian", "gptq") == (23, 20) and check_iq4_levels((), "hessian", "rtn") == ()
    with pytest.raises(ValueError, match="level_db_iq4_method"):
        check_iq4_levels(("IQ4_XS",), "hessian", "obq")
    with pytest.raises(ValueError, match="needs level_db_iq4"):
        check_iq4_levels((), "hessian", "gptq")
