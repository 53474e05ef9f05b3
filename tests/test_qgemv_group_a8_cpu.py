"""The grouped dense decode launch on int8 activations (K39), host side (no GPU): every refusal of gq_gemv_packed_group_a8 --
made before the first HIP call, so host pointers do --, each naming its argument in the header's order; the partition of the
grid on written-out cases; the export tuple against the header; and the decode_group plumbing."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")

A = 256  # any 16-byte aligned address, never dereferenced
F16, SPLIT, SWIGLU = 1, 0, 1
Q2, Q4, Q6, Q8, IQ4_NL, IQ4_XS = 10, 12, 14, 8, 20, 23
BAD_TYPE, BAD_SHAPE, NULL = -1, -2, -6
NAME = "gq_gemv_packed_group_a8"
M = dict(q_type=Q4, blocks=A, row_src=None, R=4, y=A)
PAIR = [M, dict(M, y=None)]  # a good SWIGLU pair


def call(members, n=None, C=256, x=A, T=1, x_dtype=F16, mode=SPLIT):
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()
    table = (_cabi.GemvMember * 8)(*[_cabi.GemvMember(*m.values()) for m in members])
    rc = L.gq_gemv_packed_group_a8(table, len(members) if n is None else n, C, x, T, x_dtype, mode, None)
    return rc, L.gq_last_error().decode()


# one fault per call, then pairs of faults: the earlier check of the documented order names its argument
REFUSALS = [
    (BAD_TYPE, "mode 2", dict(mode=2, n=0)),
    (BAD_SHAPE, "n_members=0", dict(n=0, x_dtype=0)),
    (BAD_SHAPE, "n_members=5", dict(members=[M] * 5)),
    (BAD_TYPE, "x_dtype 0", dict(x_dtype=0, members=[dict(M, q_type=9)])),
    (BAD_TYPE, "members[1].q_type 20 (GQ_IQ4_NL)", dict(members=[M, dict(M, q_type=IQ4_NL, blocks=None)])),
    (BAD_TYPE, "members[0].q_type 23 (GQ_IQ4_XS)", dict(members=[dict(M, q_type=IQ4_XS)])),
    (BAD_TYPE, "members[2].q_type: unknown q_type 9", dict(members=[M, M, dict(M, q_type=9)], mode=SWIGLU)),
    (BAD_SHAPE, "n_members=3 (GQ_GEMV_GROUP_SWIGLU", dict(members=[M, M, M], mode=SWIGLU)),
    (BAD_TYPE, "members[1].q_type 14 != members[0].q_type 12", dict(members=[M, dict(M, q_type=Q6)], mode=SWIGLU)),
    (BAD_SHAPE, "members[1].y is not NULL", dict(members=[M, dict(M, blocks=None)], mode=SWIGLU)),
    (NULL, "members[1].blocks is NULL", dict(members=[M, dict(M, blocks=None, y=None)], x=None)),
    (NULL, "members[0].y is NULL", dict(members=[dict(M, y=None, R=0)])),
    (NULL, "x is NULL", dict(x=None, T=5)),
    (BAD_SHAPE, "members[1].R=0", dict(members=[M, dict(M, R=0)], T=5)),
    (BAD_SHAPE, "members[1].R=5 != members[0].R=4", dict(members=[M, dict(M, R=5, y=None)], mode=SWIGLU, T=0)),
    (BAD_SHAPE, "T=5", dict(T=5, C=128)),
    (BAD_SHAPE, "C=128", dict(C=128, x=A + 2)),
    (BAD_SHAPE, "T=4 C=32768: the quantized image of x, 149504 bytes, does not fit the 131072", dict(T=4, C=32768, x=A + 2)),
    (BAD_SHAPE, "members[1].blocks not 16-byte aligned", dict(members=[M, dict(M, blocks=A + 8, y=A + 2)])),
    (BAD_SHAPE, "members[0].row_src not 4-byte aligned", dict(members=[dict(M, q_type=Q6, blocks=A + 2, row_src=A + 2)], x=A + 2)),
    (BAD_SHAPE, "members[3].y not 16-byte aligned", dict(members=[M, M, M, dict(M, y=A + 2)], T=4, C=28672)),  # the limits themselves pass
    (BAD_SHAPE, "x not 16-byte aligned", dict(members=PAIR, mode=SWIGLU, x=A + 8)),
]


@pytest.mark.parametrize("status,word,kw", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_need_no_device_and_name_the_argument(status, word, kw):
    rc, msg = call(**dict(dict(members=[M]), **kw))
    assert rc == status and msg.startswith(NAME + ": ") and word in msg, (kw, rc, msg)


@pytest.mark.parametrize("types,R,C,T,swiglu,want", [
    # Llama-3-8B's q / k / v, Q4_K: quotas 170.67, 42.67, 42.67 of 256 -> 170, 42, 42 and the two left over to q, then k
    ((Q4, Q4, Q4), (4096, 1024, 1024), 4096, 1, False, dict(lds_bytes=4672, grid=256, first_wg=[0, 171, 214, 256])),
    # the Q4_K_M-like mix, v in Q6_K (210 bytes per superblock against 144): quotas 158.55, 39.64, 57.81 -> v, then k
    ((Q4, Q4, Q6), (4096, 1024, 1024), 4096, 4, False, dict(lds_bytes=4 * 4672, grid=256, first_wg=[0, 158, 198, 256])),
    # fewer row groups than CUs: every member one workgroup per row group (quotas 3.23, 2.004, 0.76: the floor of 1)
    ((Q4, Q6, Q8), (40, 17, 5), 256, 3, False, dict(lds_bytes=3 * 292, grid=6, first_wg=[0, 3, 5, 6])),
    # two tiny members lifted to one workgroup each: 255 + 1 + 1 > 256, the big one gives one back
    ((Q4, Q2, Q2), (100000, 1, 1), 256, 1, False, dict(grid=256, first_wg=[0, 254, 255, 256])),
    ((Q4, Q4), (14336, 14336), 4096, 4, True, dict(lds_bytes=4 * 4672, grid=256, first_wg=[0, 0, 256])),
    ((Q6, Q6), (19, 19), 32768, 4, True, dict(grid=2, first_wg=[0, 0, 2], fits=False)),
])
def test_plan_is_pure_arithmetic(types, R, C, T, swiglu, want):
    from gptq_gguf_toolkit_amd import _cabi, ops
    plan = ops.gemv_group_a8_plan(types, R, C, T, swiglu)
    assert {k: plan[k] for k in want} == want and plan["fits"] == want.get("fits", True)
    for bad in (((IQ4_NL,) + types[1:], R, C, T), (types, (0,) + R[1:], C, T), (types, R, C + 128, T), (types, R, C, 5), (types * 3, R * 3, C, T)):
        with pytest.raises(_cabi.GQError, match=r"q_type 20|R=0|C=|T=5|n_members="):
            ops.gemv_group_a8_plan(*bad, swiglu)


def test_header_symbols_are_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_qgemv_group_a8.h")).read()
    assert set(re.findall(r"^int (gq_[a-z0-9_]+)\s*\(", hdr, re.M)) == set(_cabi.EXPORTS_QGEMV_GROUP_A8) == {NAME, "gq_gemv_group_a8_plan"}
    L = _cabi.lib()
    assert len(L.gq_gemv_packed_group_a8.argtypes) == 8 and len(L.gq_gemv_group_a8_plan.argtypes) == 10
    assert ctypes.sizeof(_cabi.GemvMember) == 40 and _cabi.GEMV_GROUP_MAX == 4  # gq_gemv_member_t, GQ_GEMV_GROUP_MAX
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6  # additive: the version stays
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc


def test_ops_refusals_and_the_decode_group_plumbing(tmp_path, capsys):
    from gptq_gguf_toolkit_amd import _cabi, generate, gguf_loader, ops, packed_group
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    x, b = torch.zeros(1, 256, dtype=torch.float16), torch.zeros(4 * 144, dtype=torch.uint8)
    with pytest.raises(_cabi.GQError, match="CPU"):  # every argument good but on the host: there is no CPU path
        ops.gemv_packed_group_q8([(Q4, b, None)], x)
    with pytest.raises(_cabi.GQError, match="5 members"):
        ops.gemv_packed_group_q8([(Q4, b, None)] * 5, x)
    with pytest.raises(_cabi.GQError, match="one shape and type"):
        ops.gemv_swiglu_packed_q8(Q4, b, b[:144], x)
    ids = tmp_path / "ids.pt"
    ids.write_bytes(b"")
    base = ["--model_name_or_path", "m", "--output_file", "-", "--gguf", "f.gguf", "--prompt_ids", str(ids), "--max_new_tokens", "1"]
    q8 = ["--packed", "--decode_act", "q8"]
    assert [generate.parse_args(base + q8 + a).decode_group for a in ([], ["--decode_group", "on"])] == ["off", "on"]
    for argv in (base + ["--packed", "--decode_group", "on"], base + ["--decode_group", "on"]):
        with pytest.raises(SystemExit):
            generate.parse_args(argv)
        assert "--decode_group needs --packed --decode_act q8" in capsys.readouterr().err
    with pytest.raises(ValueError, match="packed_decode_group"):
        gguf_loader.load_into_model(torch.nn.Module(), "unused.gguf", packed=True, packed_decode_group=True)

    class Attn(torch.nn.Module):
        def __init__(self, act):
            super().__init__()
            self.q_proj, self.k_proj, self.v_proj = (PackedLinear(256, 16, decode_act=act) for _ in range(3))

    model = torch.nn.Sequential(Attn("q8"), Attn("fp"))
    assert packed_group.install_groups(model) == 1 == packed_group.install_groups(model)  # idempotent; decode_act="fp" is left alone
    assert "forward" in model[0].k_proj.__dict__ and "forward" not in model[1].k_proj.__dict__
    packed_group.restore(model)
    assert not any("forward" in m.__dict__ or "decode_group" in m.__dict__ for m in model.modules())
