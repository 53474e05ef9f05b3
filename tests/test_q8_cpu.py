"""Q8_0 on the GPU, host side (no GPU): the additive header include/gptq_gguf_q8.h and its binding, every refusal of the new
type's entry points -- made before the first HIP call, so host pointers do -- the entry points that keep refusing type 8,
the --level_db_q8_0 flag's rule, and the encoder fixtures of tests/test_gpu_q8.py pinned against the scalar restatement of
ggml-quants.c (tests/ggml_spec.py)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")

P = 256  # any 16-byte aligned address, never dereferenced


def _msg(L):
    return L.gq_last_error().decode()


def test_q8_header_symbols_are_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi
    from gptq_gguf_toolkit_amd.gguf_writer import GGML_QUANT_SIZES, GGMLType
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_q8.h")).read()
    declared = set(re.findall(r"^int (gq_[a-z0-9_]+)\s*\(", hdr, re.M))  # (the comments name the decoders of other headers)
    L = _cabi.lib()
    assert declared == set(_cabi.EXPORTS_Q8) == {"gq_quantize_q8_0"}
    assert hasattr(ctypes.CDLL(_cabi.SO_PATH), "gq_quantize_q8_0") and L.gq_quantize_q8_0.argtypes
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6  # additive: the version stays
    m = re.search(r"#define GQ_Q8_0 (\d+)", hdr)
    assert m and int(m.group(1)) == _cabi.Q8_0 == int(GGMLType.Q8_0) == 8
    assert GGML_QUANT_SIZES[GGMLType.Q8_0] == (32, 34)
    assert "non-finite" in hdr  # the header says what is outside the contract
    assert "`gq_quantize_q8_0`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "gptq_gguf_q8.h" in open(os.path.join(ROOT, "README.md")).read()


def test_level_switch_takes_kind_8_and_checks_its_shape_and_alignment():
    """Before this type existed kind 8 was GQ_E_BAD_TYPE "kind 8": now its own rules speak."""
    from gptq_gguf_toolkit_amd import _cabi
    L, J = _cabi.lib(), _cabi.SwitchJob

    def refused(jobs, status, *words):
        rc = L.gq_level_switch((J * len(jobs))(*jobs), len(jobs), None)
        assert rc == status and all(w in _msg(L) for w in words), (rc, _msg(L))

    ok = J(P, P, None, 4, 256, 12, 1)
    refused([ok, J(P, P, None, 4, 48, 8, 1)], -2, "job 1", "C=48")               # Q8_0: C % 32
    refused([J(P + 1, P, None, 4, 96, 8, 1)], -2, "job 0", "src not 2-byte aligned")
    refused([J(P + 3, P, None, 4, 96, 8, 2)], -2, "job 0", "aligned")
    refused([J(P + 2, P + 8, None, 4, 96, 8, 1)], -2, "job 0", "dst not 16-byte aligned")  # src 2-byte aligned is enough
    refused([J(P, P, None, 0, 96, 8, 1)], -2, "job 0", "R=0")
    refused([J(None, P, None, 4, 96, 8, 1)], -6, "job 0", "src is NULL")
    refused([J(P, P, None, 4, 96, 8, 3)], -1, "job 0", "out_dtype 3")
    refused([J(P, P, None, 1 << 50, 96, 8, 1)], -2, "job 0", "more than one launch")
    for kind in (3, 9, 15):  # its neighbours stay unknown
        refused([J(P, P, None, 4, 256, kind, 1)], -1, "job 0", f"kind {kind}")


def test_dequantize_blocks_takes_type_8_and_checks_its_shape():
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()
    assert L.gq_dequantize_blocks(8, P, 4, 48, None, P, 1, None) == -2 and "C=48" in _msg(L)
    assert L.gq_dequantize_blocks(8, P, 0, 96, None, P, 1, None) == -2
    assert L.gq_dequantize_blocks(8, P + 1, 4, 96, None, P, 1, None) == -2 and "2-byte aligned" in _msg(L)
    assert L.gq_dequantize_blocks(8, P + 2, 4, 96, None, P + 4, 1, None) == -2 and "16-byte aligned" in _msg(L)
    assert L.gq_dequantize_blocks(8, None, 4, 96, None, P, 1, None) == -6
    assert L.gq_dequantize_blocks(8, P, 4, 96, None, P, 5, None) == -1 and "out_dtype 5" in _msg(L)
    assert L.gq_dequantize_blocks(12, P, 4, 96, None, P, 1, None) == -2 and "C=96" in _msg(L)  # a K-quant still needs 256
    for q_type in (3, 9, 15):
        assert L.gq_dequantize_blocks(q_type, P, 4, 256, None, P, 1, None) == -1 and f"q_type {q_type}" in _msg(L)


def test_quantize_q8_0_argument_checks_need_no_device():
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()
    q = L.gq_quantize_q8_0
    assert q(P, 0, 4, 40, None, P, None) == -2 and "C=40" in _msg(L)
    assert q(P, 0, 4, 0, None, P, None) == -2 and q(P, 0, 0, 64, None, P, None) == -2 and "R=0" in _msg(L)
    assert q(P, 0, 4, 1 << 31, None, P, None) == -2
    assert q(P, 7, 4, 64, None, P, None) == -1 and "x_dtype 7" in _msg(L)
    assert q(P, 8, 4, 64, None, P, None) == -1  # (a quantized type is no input dtype)
    assert q(None, 0, 4, 64, None, P, None) == -6 and q(P, 1, 4, 64, None, None, None) == -6 and "null" in _msg(L)
    assert q(P + 8, 2, 4, 64, None, P, None) == -2 and "16-byte aligned" in _msg(L)
    assert q(P, 2, 4, 64, None, P + 2, None) == -2 and "16-byte aligned" in _msg(L)
    assert q(P, 2, 4, 64, P + 2, P, None) == -2 and "row_src" in _msg(L)


def test_every_other_entry_point_keeps_refusing_type_8():
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()
    assert L.gq_pack(8, P, P, P, P, P, 4, 256, P, None) == -1 and "q_type 8" in _msg(L)
    assert L.gq_unpack(8, P, 4, 256, P, P, P, P, P, None) == -1 and "q_type 8" in _msg(L)
    assert L.gq_type_info(8, ctypes.byref(_cabi.TypeInfo())) == -1
    s = _cabi.Search(-1.0, 0.1, 20, 0, 100, 0.8)
    assert L.gq_rtn_quantize(P, 0, 4, 256, 8, ctypes.byref(s), P, P, P, P, P, None) == -1
    bands = (_cabi.Band * 1)(_cabi.Band(64, 8))
    outs = (ctypes.c_void_p * 1)(P)
    assert L.gq_pack_bands(P, P, P, P, P, 64, 256, bands, 1, outs, None, None) == -1
    assert L.gq_gptq_quantize_bands(P, P, 64, 256, bands, 1, 128, ctypes.byref(s), P, P, P, P, P, P, 1 << 30, None) == -1


def test_ops_refuse_a_q8_0_source_of_the_wrong_size():
    from gptq_gguf_toolkit_amd import _cabi, ops
    assert ops.block_geometry(8) == (32, 34) and ops.block_geometry(12) == (256, 144)
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.quantize_q8_0(torch.zeros(4, 64))
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.dequantize_blocks(8, torch.zeros(4, 68, dtype=torch.uint8))


def test_level_db_q8_0_flag_needs_a_level_db(monkeypatch, capsys, tmp_path):
    from gptq_gguf_toolkit_amd.quant import levels_problem, parse_args
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    model = tmp_path / "model"
    model.mkdir()
    base = ["--model_name_or_path", str(model), "--quantizable_modules", "x", "--pre_block_modules", "e", "--block_modules", "b",
            "--calibration_data", "c.pt", "--save_dir", "s"]
    lv = ["--levels", "Q2_K", "Q4_K", "--propagate_level", "Q4_K"]
    for extra in (["--level_db_q8_0"], lv + ["--level_db_q8_0"]):
        with pytest.raises(SystemExit) as e:
            parse_args(base + extra)
        assert e.value.code == 2 and "--level_db_q8_0 needs --level_db" in capsys.readouterr().err
    a = parse_args(base + lv + ["--level_db", str(tmp_path / "db"), "--level_db_q8_0"])
    assert a.level_db_q8_0 is True and levels_problem(a) is None
    assert parse_args(base + lv + ["--level_db", str(tmp_path / "db")]).level_db_q8_0 is False
    ns = types.SimpleNamespace(levels=None, propagate_level=None, level_db=None, level_db_only=False, level_db_q8_0=True)
    assert "--level_db_q8_0 needs --level_db" in levels_problem(ns)
    with pytest.raises(SystemExit):  # Q8_0 is a level of the database, never one of --levels
        parse_args(base + ["--levels", "Q8_0", "--propagate_level", "none"])
    assert "invalid choice" in capsys.readouterr().err


def test_quantize_levels_refuses_the_flag_without_a_database():
    from gptq_gguf_toolkit_amd.quantizer import Quantizer
    drv = Quantizer.__new__(Quantizer)
    drv.quantizer_kwargs = {}
    with pytest.raises(ValueError, match="level_db_q8_0 needs level_db"):
        drv.quantize_levels([10, 12], 12, level_db=None, level_db_q8_0=True)


def test_encoder_fixtures_are_pinned_on_the_host():
    """The reference of the GPU encoder test is gguf_writer.quantize_q8_0: here it is held against the element-by-element
    restatement of quantize_row_q8_0_ref on the crafted blocks, and the properties the GPU test relies on are checked."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import q8_cases as Q
    from ggml_spec import q8_0_encode_scalar
    from gptq_gguf_toolkit_amd.gguf_writer import quantize_q8_0
    x = Q.crafted_encoder_matrix()
    with np.errstate(over="ignore"):
        got = quantize_q8_0(x)
        assert got.shape == (4, 34) and got.tobytes() == q8_0_encode_scalar(x)
    codes = got[:, 2:].view(np.int8)
    d = got[:, :2].copy().view(np.float16).ravel()
    assert codes[0, :9].tolist() == Q.HALVES_AWAY != Q.HALVES_EVEN and not codes[0, 9:].any() and d[0] == 1.0
    assert not got[1].any() and np.signbit(x[1, 5])                       # the -0.0 block: d = +0, codes 0
    assert np.isinf(d[2]) and np.abs(codes[2]).max() == 127               # d overflows fp16, the codes do not care
    assert 0 < d[3] < np.float16(6.104e-5) and np.abs(codes[3]).max() == 127   # an fp16 subnormal
    r = Q.random_encoder_matrix()
    hit = Q.division_and_reciprocal_differ(r)
    assert r.shape == (2048, 1024) and hit.size >= 1
    blk = r.reshape(-1, 32)[hit[:4]]
    assert quantize_q8_0(blk).tobytes() == q8_0_encode_scalar(blk)        # ... and there the reference multiplies by id
