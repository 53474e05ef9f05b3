"""The packed MoE decode step on int8 activations, host side (no GPU): every refusal of gq_gemv_packed_experts_a8 -- made
before the first HIP call, so host pointers do --, each naming its argument; the plan's pure arithmetic; the export tuple
against the header; and the decode_act plumbing."""
import os
import re

import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")

A = 256  # any 16-byte aligned address, never dereferenced
F16 = 1
BAD_TYPE, BAD_SHAPE, NULL = -1, -2, -6
NAME = "gq_gemv_packed_experts_a8"
ARGS = dict(q_type=12, blocks=A, E=3, R=4, C=256, x=A, x_up=None, x_rows=2, pe=A, P=4, ppr=2, x_dtype=F16, y=A)

# one fault per call, then pairs of faults: the earlier check of the documented order names its argument
REFUSALS = [
    (BAD_TYPE, "q_type 9", dict(q_type=9)),
    (BAD_TYPE, "GQ_IQ4_NL", dict(q_type=20, x_dtype=0)),
    (BAD_TYPE, "GQ_IQ4_XS", dict(q_type=23)),
    (BAD_TYPE, "x_dtype 0", dict(x_dtype=0, blocks=None)),
    (NULL, "pair_expert is NULL", dict(pe=None, E=0)),
    (BAD_SHAPE, "E=0", dict(E=0, R=0)),
    (BAD_SHAPE, "R=0", dict(R=0, P=0)),
    (BAD_SHAPE, "P=0", dict(P=0, x_rows=0)),
    (BAD_SHAPE, "P=65", dict(P=65, x_rows=65, ppr=1)),
    (BAD_SHAPE, "x_rows=3 * pairs_per_row=2 != P=4", dict(x_rows=3, C=128)),
    (BAD_SHAPE, "C=128", dict(C=128, y=A + 2)),
    (BAD_SHAPE, "P=4 C=32768: the quantized image of 4 rows of x, 149504 bytes, does not fit the 131072", dict(C=32768, x=A + 2)),
    (BAD_SHAPE, "blocks not 16-byte aligned", dict(blocks=A + 8, x_up=A + 8)),
    (BAD_SHAPE, "x_up not 16-byte aligned", dict(x_up=A + 8, y=A + 2)),
    (BAD_SHAPE, "y not 16-byte aligned", dict(E=65535, P=64, x_rows=64, ppr=1, C=28672, x_up=A, y=A + 2)),  # the limits themselves pass
]


@pytest.mark.parametrize("status,word,kw", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_need_no_device_and_name_the_argument(status, word, kw):
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()
    rc = L.gq_gemv_packed_experts_a8(*dict(ARGS, **kw).values(), None)
    msg = L.gq_last_error().decode()
    assert rc == status and msg.startswith(NAME + ": ") and word in msg, (kw, rc, msg)


@pytest.mark.parametrize("P,R,C,want", [
    (1, 1, 256, dict(lds_bytes=292, rows_per_turn=16, grid_x=1, fits=True)),                  # 256 * 73 / 64
    (2, 14336, 4096, dict(lds_bytes=2 * 4672, rows_per_turn=16, grid_x=128, fits=True)),      # Mixtral's gate at T = 1: capped
    (64, 4096, 14336, dict(lds_bytes=4 * 16352, rows_per_turn=16, grid_x=128, fits=True)),    # min(P, 4) rows
    (3, 130, 32768, dict(lds_bytes=3 * 37376, rows_per_turn=16, grid_x=9, fits=True)),        # three rows of it fit, four do not
])
def test_plan_is_pure_arithmetic(P, R, C, want):
    from gptq_gguf_toolkit_amd import _cabi, ops
    plan = ops.gemv_experts_a8_plan(P, R, C)
    assert plan["grid_x_cap"] == 128 and {k: plan[k] for k in want} == want
    for bad in ((0, R, C), (65, R, C), (P, 0, C), (P, R, C + 128)):
        with pytest.raises(_cabi.GQError, match="P=|R=|C="):
            ops.gemv_experts_a8_plan(*bad)


def test_header_symbols_are_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_moe_gemv_a8.h")).read()
    assert set(re.findall(r"^int (gq_[a-z0-9_]+)\s*\(", hdr, re.M)) == set(_cabi.EXPORTS_MOE_GEMV_A8) == {NAME, "gq_gemv_experts_a8_plan"}
    L = _cabi.lib()
    assert len(L.gq_gemv_packed_experts_a8.argtypes) == 14 and len(L.gq_gemv_experts_a8_plan.argtypes) == 8
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6  # additive: the version stays
    for doc in ("README.md", "DESIGN.md"):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc


def test_ops_refusals_and_the_decode_act_plumbing(tmp_path, capsys):
    from gptq_gguf_toolkit_amd import _cabi, generate, gguf_loader, ops
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts, replace_experts
    E, R, C = 3, 4, 256
    good = dict(q_type=12, blocks=torch.zeros(E * R * 144, dtype=torch.uint8), E=E, R=R, x=torch.zeros(2, C, dtype=torch.float16),
                pair_expert=torch.zeros(4, dtype=torch.int32), pairs_per_row=2)
    for kw, word in ((dict(q_type=23), "q_type 23 is not served"),
                     (dict(x_up=torch.zeros(2, C, dtype=torch.bfloat16)), "x_up must be"),
                     (dict(pairs_per_row=1), r"x_rows=2 \* pairs_per_row=1 != P=4"),
                     (dict(), "CPU")):  # every argument good but on the host: there is no CPU path
        with pytest.raises(_cabi.GQError, match=word):
            ops.gemv_packed_experts_q8(**dict(good, **kw))
    ids = tmp_path / "ids.pt"
    ids.write_bytes(b"")
    base = ["--model_name_or_path", "m", "--output_file", "-", "--gguf", "f.gguf", "--prompt_ids", str(ids), "--max_new_tokens", "1"]
    assert [generate.parse_args(base + ["--packed"] + a).moe_decode_act for a in ([], ["--moe_decode_act", "q8"])] == ["fp", "q8"]
    with pytest.raises(SystemExit):
        generate.parse_args(base + ["--moe_decode_act", "q8"])
    assert "--moe_decode_act needs --packed" in capsys.readouterr().err
    holder = torch.nn.Module()
    with pytest.raises(ValueError, match="moe_decode_act"):
        gguf_loader.load_into_model(holder, "unused.gguf", moe_decode_act="q8")
    with pytest.raises(ValueError, match="moe_decode_act"):
        LevelStore(holder, str(tmp_path), "cpu", moe_decode_act="q8")
    with pytest.raises(ValueError, match="decode_act must be 'fp' or 'q8'"):
        replace_experts(holder, "mlp", decode_act="int8")
    mod = PackedExperts(4, 256, 256)
    mod.decode_act = "int8"
    for r in ("gate", "up", "down"):
        mod.set_level(r, torch.zeros(4 * 256 * 144, dtype=torch.uint8), 12)
    with pytest.raises(_cabi.GQError, match="decode_act must be 'fp' or 'q8'"):
        mod(torch.zeros(1, 256, dtype=torch.float16), torch.zeros(1, 2, dtype=torch.long), torch.zeros(1, 2, dtype=torch.float16))
