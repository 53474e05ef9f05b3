"""The packed forward on int8 activations, host side (no GPU): every refusal of gq_quantize_act_q8 and gq_linear_packed_a8 --
made before the first HIP call, so host pointers do --, each naming its argument, and the command-line flag."""
import pytest

torch = pytest.importorskip("torch")

P = 256  # any 16-byte aligned address, never dereferenced
F16 = 1
BAD_TYPE, BAD_SHAPE, NULL = -1, -2, -6

QUANT = dict(x=P, T=3, C=256, x_dtype=F16, xq=P, xd=P, xbsum=P)
GEMM = dict(q_type=12, blocks=P, row_src=None, R=4, C=256, xq=P, xd=P, xbsum=P, T=3, y=P, y_dtype=F16)


def call(L, name, kw):
    a = dict(QUANT if name == "gq_quantize_act_q8" else GEMM, **kw)
    if name == "gq_quantize_act_q8":
        rc = L.gq_quantize_act_q8(a["x"], a["T"], a["C"], a["x_dtype"], a["xq"], a["xd"], a["xbsum"], None)
    else:
        rc = L.gq_linear_packed_a8(a["q_type"], a["blocks"], a["row_src"], a["R"], a["C"], a["xq"], a["xd"], a["xbsum"], a["T"],
                                   a["y"], a["y_dtype"], None)
    return rc, L.gq_last_error().decode()


# one fault per call, then pairs of faults: the earlier check of the documented order names its argument
REFUSALS = [
    ("gq_quantize_act_q8", BAD_TYPE, "x_dtype 0", dict(x_dtype=0)),
    ("gq_quantize_act_q8", BAD_SHAPE, "C=128", dict(C=128)),
    ("gq_quantize_act_q8", BAD_SHAPE, "more than one launch", dict(T=(1 << 31) - 1, C=(1 << 31) - 256)),
    ("gq_quantize_act_q8", BAD_SHAPE, "xq not 16-byte aligned", dict(xq=P + 8, xbsum=P + 2)),
    ("gq_quantize_act_q8", NULL, "xq is NULL", dict(xq=None, T=0)),
    ("gq_quantize_act_q8", BAD_SHAPE, "T=0", dict(T=0, C=100)),
    ("gq_linear_packed_a8", BAD_TYPE, "q_type 9", dict(q_type=9)),
    ("gq_linear_packed_a8", BAD_TYPE, "GQ_IQ4_XS", dict(q_type=23)),
    ("gq_linear_packed_a8", BAD_TYPE, "y_dtype 0", dict(y_dtype=0)),
    ("gq_linear_packed_a8", NULL, "blocks is NULL", dict(blocks=None)),
    ("gq_linear_packed_a8", BAD_SHAPE, "blocks not 2-byte aligned", dict(q_type=14, blocks=P + 1)),
    ("gq_linear_packed_a8", BAD_SHAPE, "row_src not 4-byte aligned", dict(row_src=P + 2)),
    ("gq_linear_packed_a8", BAD_SHAPE, "xbsum not 16-byte aligned", dict(xbsum=P + 2)),
    ("gq_linear_packed_a8", BAD_TYPE, "y_dtype 0", dict(y_dtype=0, blocks=None)),
    ("gq_linear_packed_a8", NULL, "xq is NULL", dict(xq=None, R=0)),
    ("gq_linear_packed_a8", BAD_SHAPE, "R=0", dict(R=0, T=0)),
    ("gq_linear_packed_a8", BAD_SHAPE, "T=0", dict(T=0, C=128)),
    ("gq_linear_packed_a8", BAD_SHAPE, "C=128", dict(C=128, y=P + 2)),
]


@pytest.mark.parametrize("name,status,word,kw", REFUSALS, ids=[f"{r[0][3:]}-{i}" for i, r in enumerate(REFUSALS)])
def test_refusals_need_no_device_and_name_the_argument(name, status, word, kw):
    from gptq_gguf_toolkit_amd import _cabi
    rc, msg = call(_cabi.lib(), name, kw)
    assert rc == status and msg.startswith(name + ": ") and word in msg, (kw, rc, msg)


def test_packed_act_flag_is_refused_without_packed(tmp_path, capsys):
    from gptq_gguf_toolkit_amd import evo_quant_search, ppleval
    ids = tmp_path / "ids.pt"
    ids.write_bytes(b"")
    pbase = ["--model_name_or_path", "m", "--eval_datasets", str(ids), "--output_file", str(tmp_path / "o.json"), "--gguf", "f.gguf"]
    assert [ppleval.parse_args(pbase + ["--packed"] + a).packed_act for a in ([], ["--packed_act", "q8"])] == ["fp", "q8"]
    with pytest.raises(SystemExit):
        ppleval.parse_args(pbase + ["--packed_act", "q8"])
    assert "--packed_act needs --packed" in capsys.readouterr().err
    sbase = ["--model_name_or_path", "m", "--calibration_data", str(ids), "--eval_datasets", str(ids), "--generations", "1",
             "--offspring", "2", "--target_bitwidth", "4", "--quant_weights_path", str(tmp_path), "--survivors_per_selection", "1",
             "--tokens_per_selection", "8"]
    assert evo_quant_search.parse_args(sbase + ["--resident", "packed", "--packed_act", "q8"]).packed_act == "q8"
    with pytest.raises(SystemExit):
        evo_quant_search.parse_args(sbase + ["--packed_act", "q8"])
    assert "--packed_act needs --resident packed" in capsys.readouterr().err
