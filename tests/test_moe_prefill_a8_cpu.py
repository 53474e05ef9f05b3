"""The packed MoE prefill on int8 activations, host side (no GPU): every refusal of gq_linear_packed_experts_a8 and
gq_silu_mul_quantize_act_q8 -- made before the first HIP call, so host pointers do --, each naming its argument; the export
tuple against the header; the ops' refusals; and the --moe_act flag."""
import os
import re

import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")

A = 256  # any 16-byte aligned address, never dereferenced
F16 = 1
BAD_TYPE, BAD_SHAPE, NULL = -1, -2, -6
GEMM, FUSED = "gq_linear_packed_experts_a8", "gq_silu_mul_quantize_act_q8"
ARGS = {GEMM: dict(q_type=12, blocks=A, E=3, R=4, C=256, xq=A, xd=A, xbsum=A, x_rows=2, ppr=2, es=A, order=A, P=4, y=A, y_dtype=F16),
        FUSED: dict(gate=A, up=A, P=3, I=256, dtype=F16, xq=A, xd=A, xbsum=A)}

# one fault per call, then pairs of faults: the earlier check of the documented order names its argument
REFUSALS = [
    (GEMM, BAD_TYPE, "q_type 9", dict(q_type=9)),
    (GEMM, BAD_TYPE, "GQ_IQ4_XS", dict(q_type=23)),
    (GEMM, BAD_TYPE, "GQ_IQ4_NL", dict(q_type=20, y_dtype=0)),
    (GEMM, BAD_TYPE, "y_dtype 0", dict(y_dtype=0, blocks=None)),
    (GEMM, NULL, "blocks is NULL", dict(blocks=None)),
    (GEMM, NULL, "xbsum is NULL", dict(xbsum=None, E=0)),
    (GEMM, NULL, "order is NULL", dict(order=None)),
    (GEMM, BAD_SHAPE, "E=0", dict(E=0, R=0)),
    (GEMM, BAD_SHAPE, "E=257", dict(E=257)),
    (GEMM, BAD_SHAPE, "R=0", dict(R=0, P=0)),
    (GEMM, BAD_SHAPE, "P=0", dict(P=0, x_rows=0)),
    (GEMM, BAD_SHAPE, "P=131073", dict(P=131073, x_rows=131073, ppr=1)),
    (GEMM, BAD_SHAPE, "x_rows=3 * pairs_per_row=2 != P=4", dict(x_rows=3, C=128)),
    (GEMM, BAD_SHAPE, "C=128", dict(C=128, xbsum=A + 2)),
    (GEMM, BAD_SHAPE, "blocks not 16-byte aligned", dict(blocks=A + 8)),
    (GEMM, BAD_SHAPE, "order not 4-byte aligned", dict(order=A + 2, xq=A + 8)),
    (GEMM, BAD_SHAPE, "xbsum not 16-byte aligned", dict(xbsum=A + 2, y=A + 2)),
    (GEMM, BAD_SHAPE, "y not 16-byte aligned", dict(E=256, P=131072, x_rows=131072, ppr=1, y=A + 2)),  # the limits themselves pass
    (FUSED, BAD_TYPE, "dtype 0", dict(dtype=0, gate=None)),
    (FUSED, NULL, "up is NULL", dict(up=None, P=0)),
    (FUSED, BAD_SHAPE, "P=0", dict(P=0, I=128)),
    (FUSED, BAD_SHAPE, "I=128", dict(I=128, gate=A + 8)),
    (FUSED, BAD_SHAPE, "more than one launch", dict(P=(1 << 31) - 1, I=(1 << 31) - 256)),
    (FUSED, BAD_SHAPE, "up not 16-byte aligned", dict(up=A + 8, xbsum=A + 2)),
    (FUSED, BAD_SHAPE, "xbsum not 16-byte aligned", dict(xbsum=A + 2)),
]


@pytest.mark.parametrize("name,status,word,kw", REFUSALS, ids=[f"{r[0][3:]}-{i}" for i, r in enumerate(REFUSALS)])
def test_refusals_need_no_device_and_name_the_argument(name, status, word, kw):
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()
    rc = getattr(L, name)(*dict(ARGS[name], **kw).values(), None)
    msg = L.gq_last_error().decode()
    assert rc == status and msg.startswith(name + ": ") and word in msg, (kw, rc, msg)


def test_header_symbols_are_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_moe_gemm_a8.h")).read()
    assert set(re.findall(r"^int (gq_[a-z0-9_]+)\s*\(", hdr, re.M)) == set(_cabi.EXPORTS_MOE_GEMM_A8) == {GEMM, FUSED}
    L = _cabi.lib()
    assert len(L.gq_linear_packed_experts_a8.argtypes) == 16 and len(L.gq_silu_mul_quantize_act_q8.argtypes) == 9
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6  # additive: the version stays
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert GEMM in text and FUSED in text, doc


def test_ops_refusals_name_the_value():
    from gptq_gguf_toolkit_amd import _cabi, ops
    E, R, C = 3, 4, 256
    good = dict(q_type=12, blocks=torch.zeros(E * R * 144, dtype=torch.uint8), E=E, R=R, xq=torch.zeros(2, C, dtype=torch.int8),
                xd=torch.zeros(2, 1), xbsum=torch.zeros(2, 16, dtype=torch.int16),
                route=(torch.zeros(E + 1, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)), pairs_per_row=2,
                out_dtype=torch.float16)
    for kw, word in ((dict(q_type=23), "q_type 23 is not served"),
                     (dict(out_dtype=torch.float32), "out_dtype"),
                     (dict(xq=torch.zeros(2, C, dtype=torch.float16)), "int8 codes"),
                     (dict(pairs_per_row=1), r"x_rows=2 \* pairs_per_row=1 != P=4"),
                     (dict(xd=torch.zeros(2, 2)), r"fp32 \[2, 1\]"),
                     (dict(xbsum=torch.zeros(2, 16, dtype=torch.int32)), r"int16 \[2, 16\]"),
                     (dict(), "CPU")):  # every argument good but on the host: there is no CPU path
        with pytest.raises(_cabi.GQError, match=word):
            ops.linear_packed_experts_a8(**dict(good, **kw))
    g = torch.zeros(2, C, dtype=torch.float16)
    for args, word in (((g.float(), g.float()), "fp16 or both bf16"), ((g, g.bfloat16()), "fp16 or both bf16"),
                       ((g[:, :128], g[:, :128]), "I % 256 == 0"), ((g, g[:1]), "one shape"), ((g, g), "CPU")):
        with pytest.raises(_cabi.GQError, match=word):
            ops.silu_mul_quantize_act_q8(*args)


def test_moe_act_is_carried_and_refused_without_the_grouped_prefill(tmp_path, capsys):
    from gptq_gguf_toolkit_amd import evo_quant_search, generate, gguf_loader, ppleval
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts, replace_experts
    ids = tmp_path / "ids.pt"
    ids.write_bytes(b"")
    base = ["--model_name_or_path", "m", "--output_file", str(tmp_path / "o.json"), "--gguf", "f.gguf", "--packed"]
    for mod, extra in ((ppleval, ["--eval_datasets", str(ids)]), (generate, ["--prompt_ids", str(ids), "--max_new_tokens", "1"])):
        grouped = base + extra + ["--moe_prefill", "grouped"]
        assert [mod.parse_args(grouped + a).moe_act for a in ([], ["--moe_act", "q8"])] == ["fp", "q8"]
        with pytest.raises(SystemExit):
            mod.parse_args(base + extra + ["--moe_act", "q8"])
        assert "--moe_act needs --moe_prefill grouped" in capsys.readouterr().err
    sbase = ["--model_name_or_path", "m", "--calibration_data", str(ids), "--eval_datasets", str(ids), "--generations", "1",
             "--offspring", "2", "--target_bitwidth", "4", "--quant_weights_path", str(tmp_path), "--survivors_per_selection", "1",
             "--tokens_per_selection", "8", "--resident", "packed"]
    assert evo_quant_search.parse_args(sbase + ["--moe_prefill", "grouped", "--moe_act", "q8"]).moe_act == "q8"
    with pytest.raises(SystemExit):
        evo_quant_search.parse_args(sbase + ["--moe_act", "q8"])
    assert "--moe_act needs --resident packed --moe_prefill grouped" in capsys.readouterr().err
    holder = torch.nn.Module()
    with pytest.raises(ValueError, match="moe_act"):
        gguf_loader.load_into_model(holder, "unused.gguf", packed=True, moe_act="q8")
    with pytest.raises(ValueError, match="moe_act"):
        LevelStore(holder, str(tmp_path), "cpu", resident="packed", moe_act="q8")
    with pytest.raises(ValueError, match="'fp' or 'q8'"):
        replace_experts(holder, "mlp", "grouped", "int8")
    assert PackedExperts.act == "fp" and PackedExperts(4, 256, 256).act == "fp"
