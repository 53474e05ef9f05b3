"""The packed-weight forward, host side (no GPU): the additive header include/gptq_gguf_qgemm.h and its binding, every
refusal of gq_linear_packed -- made before the first HIP call, so host pointers do --, the capacity arithmetic of packed
residency on invented sizes, the level store's pass-1 refusal of a database packed residency cannot hold, and the new flags."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")

P = 256  # any 16-byte aligned address, never dereferenced
F16, BF16 = 1, 2
BAD_TYPE, BAD_SHAPE, NULL = -1, -2, -6


def _msg(L):
    return L.gq_last_error().decode()


def test_qgemm_header_symbol_is_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_qgemm.h")).read()
    declared = set(re.findall(r"^int (gq_[a-z0-9_]+)\s*\(", hdr, re.M))
    L = _cabi.lib()
    assert declared == set(_cabi.EXPORTS_QGEMM) == {"gq_linear_packed"}
    assert hasattr(ctypes.CDLL(_cabi.SO_PATH), "gq_linear_packed") and len(L.gq_linear_packed.argtypes) == 10
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6 and len(_cabi.EXPORTS) == 48  # additive: the version stays
    for word in ("C % 256 == 0", "Deterministic", "summation order", "Nothing outside [y, y + T * R * 2)"):
        assert word in hdr, word
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "gptq_gguf_qgemm.h" in text and "gq_linear_packed" in text, doc


def test_linear_packed_refusals_need_no_device():
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()

    def call(q_type=12, blocks=P, row_src=None, R=4, C=256, x=P, T=3, x_dtype=F16, y=P):
        return L.gq_linear_packed(q_type, blocks, row_src, R, C, x, T, x_dtype, y, None)

    def refused(status, word, **kw):
        rc = call(**kw)
        assert rc == status and word in _msg(L), (kw, rc, _msg(L))

    refused(BAD_SHAPE, "C=128", C=128)
    refused(BAD_SHAPE, "C=288", q_type=8, C=288)          # Q8_0 too: a multiple of 32 is not enough here
    refused(BAD_SHAPE, "C=0", C=0)
    refused(BAD_SHAPE, "R=0", R=0)
    refused(BAD_SHAPE, "T=0", T=0)
    refused(BAD_TYPE, "x_dtype 0", x_dtype=0)             # fp32 activations: no such path
    refused(BAD_TYPE, "x_dtype 3", x_dtype=3)
    for q_type in (3, 9, 15, 0, 1, 2):
        refused(BAD_TYPE, f"q_type {q_type}", q_type=q_type)
    # the block's natural alignment per type: Q2_K 4, Q3_K / Q6_K / Q8_0 2, Q4_K / Q5_K 16
    for q_type, ok, bad, al in ((10, P + 4, P + 2, 4), (11, P + 2, P + 1, 2), (12, P + 16, P + 8, 16), (13, P + 16, P + 4, 16),
                                (14, P + 6, P + 3, 2), (8, P + 2, P + 1, 2)):
        refused(BAD_SHAPE, f"blocks not {al}-byte aligned", q_type=q_type, blocks=bad)
        refused(BAD_SHAPE, "x not 16-byte aligned", q_type=q_type, blocks=ok, x=P + 8)  # (aligned enough: on to the next check)
    refused(BAD_SHAPE, "x not 16-byte aligned", x=P + 8)
    refused(BAD_SHAPE, "y not 16-byte aligned", y=P + 2)
    refused(BAD_SHAPE, "row_src not 4-byte aligned", row_src=P + 2)
    refused(NULL, "blocks is NULL", blocks=None)
    refused(NULL, "x is NULL", x=None)
    refused(NULL, "y is NULL", y=None)
    refused(BAD_SHAPE, "more than one launch", R=(1 << 31) - 1, T=(1 << 31) - 1)


def test_linear_packed_names_the_earlier_of_two_faults():
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()
    for status, word, kw in ((BAD_TYPE, "q_type 9", dict(q_type=9, x=None)),
                             (BAD_TYPE, "x_dtype 0", dict(x_dtype=0, blocks=None)),
                             (NULL, "x is NULL", dict(x=None, C=128)),
                             (BAD_SHAPE, "R=0 (not in [1, 2^31))", dict(R=0, C=128)),
                             (BAD_SHAPE, "C=128 (C % 256 != 0 or not in [256, 2^31); Q8_0 and IQ4_NL included)", dict(C=128, y=P + 2)),
                             (BAD_SHAPE, "blocks not 16-byte aligned", dict(blocks=P + 8, x=P + 8))):
        args = dict(q_type=12, blocks=P, row_src=None, R=4, C=256, x=P, T=3, x_dtype=F16, y=P)
        args.update(kw)
        rc = L.gq_linear_packed(args["q_type"], args["blocks"], args["row_src"], args["R"], args["C"], args["x"], args["T"],
                                args["x_dtype"], args["y"], None)
        assert rc == status and _msg(L).startswith("gq_linear_packed: ") and word in _msg(L), (kw, rc, _msg(L))


def test_ops_linear_packed_refuses_cpu_tensors():
    from gptq_gguf_toolkit_amd import _cabi, ops
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.linear_packed(12, torch.zeros(4, 144, dtype=torch.uint8), torch.zeros(3, 256, dtype=torch.float16))


def test_packed_capacity_arithmetic():
    from gptq_gguf_toolkit_amd.level_store import packed_fits, packed_peak_bytes
    # two Linears, 100 bytes dense each, levels of 150 each; 100 bytes free: 300 > 100, but each upload follows its own free
    assert packed_peak_bytes([150, 150], [100, 100]) == 100 and packed_fits([150, 150], [100, 100], 100)
    assert not packed_fits([150, 150], [0, 0], 100)            # ... without the credit (dense residency's rule) it does not fit
    assert not packed_fits([150, 150], [100, 100], 99)         # and one byte less is refused
    assert packed_peak_bytes([400, 10], [100, 100]) == 300     # the peak is met on the way, not at the end (210)
    assert packed_peak_bytes([10, 10], [100, 100]) == -90 and packed_fits([10, 10], [100, 100], 0)  # a model that only shrinks
    assert packed_peak_bytes([], []) == 0
    # Llama-3-70B on one 288 GB device: 70e9 parameters, Q2_K .. Q6_K + Q8_0 = 31.1 bits each, the live model 16 bits
    n, hbm = 70e9, 288e9
    levels, dense = n * 31.1 / 8, n * 16 / 8
    assert round((levels + dense) / 1e9) == 412 and levels + dense > hbm      # dense residency: refused
    assert round(levels / 1e9) == 272 and round(n * 22.6 / 8 / 1e9) == 198    # what is left without the dense copy
    free_with_model_loaded = hbm - dense
    assert not levels <= free_with_model_loaded                               # LevelStore's dense rule: MemoryError
    blocks = 80
    assert packed_fits([levels / blocks] * blocks, [dense / blocks] * blocks, free_with_model_loaded)
    assert packed_peak_bytes([levels / blocks] * blocks, [dense / blocks] * blocks) == pytest.approx(levels - dense)


def test_packed_store_refuses_torch_saved_levels_before_any_upload(tmp_path, monkeypatch):
    from gptq_gguf_toolkit_amd import level_store
    model = torch.nn.Sequential()
    model.add_module("lin", torch.nn.Linear(256, 8, bias=False).half())
    (tmp_path / "lin").mkdir()
    torch.save(torch.zeros(8, 256, dtype=torch.float16), str(tmp_path / "lin" / "4-Q4_K.pth"))

    def no_upload(self, name, lv):
        raise AssertionError("an upload was started")

    monkeypatch.setattr(level_store.LevelStore, "_upload", no_upload)
    with pytest.raises(ValueError, match=r"4-Q4_K\.pth.*dense residency"):
        level_store.LevelStore(model, str(tmp_path), "cpu", ["lin"], resident="packed")
    assert type(model.lin) is torch.nn.Linear and model.lin.weight.shape == (8, 256)  # nothing was freed either
    with pytest.raises(ValueError, match="resident"):
        level_store.LevelStore(model, str(tmp_path), "cpu", ["lin"], resident="sparse")
    with pytest.raises(AssertionError, match="an upload was started"):  # dense residency takes the same database
        level_store.LevelStore(model, str(tmp_path), "cpu", ["lin"])
    with pytest.raises(TypeError, match="fp16 / bf16"):
        level_store.LevelStore(model.float(), str(tmp_path), "cpu", ["lin"], resident="packed")


def test_error_estimator_refuses_a_packed_store():
    import types
    from gptq_gguf_toolkit_amd.error_estimator import ErrorEstimator
    with pytest.raises(ValueError, match="packed-resident"):
        ErrorEstimator(None, [], "", [], "", "", level_store=types.SimpleNamespace(resident="packed"))


def test_new_flags_parse_and_default_to_dense(tmp_path, capsys):
    from gptq_gguf_toolkit_amd import evo_quant_search, ppleval
    ids = tmp_path / "ids.pt"
    ids.write_bytes(b"")
    base = ["--model_name_or_path", "m", "--calibration_data", str(ids), "--eval_datasets", str(ids), "--generations", "1",
            "--offspring", "2", "--target_bitwidth", "4", "--quant_weights_path", str(tmp_path), "--survivors_per_selection", "1",
            "--tokens_per_selection", "8"]
    assert evo_quant_search.parse_args(base).resident == "dense"
    assert evo_quant_search.parse_args(base + ["--resident", "packed"]).resident == "packed"
    with pytest.raises(SystemExit):
        evo_quant_search.parse_args(base + ["--resident", "sparse"])
    assert "invalid choice" in capsys.readouterr().err
    pbase = ["--model_name_or_path", "m", "--eval_datasets", str(ids), "--output_file", str(tmp_path / "o.json")]
    assert ppleval.parse_args(pbase + ["--gguf", "f.gguf"]).packed is False
    assert ppleval.parse_args(pbase + ["--gguf", "f.gguf", "--packed"]).packed is True
    with pytest.raises(SystemExit):
        ppleval.parse_args(pbase + ["--packed"])
    assert "--packed needs --gguf" in capsys.readouterr().err
