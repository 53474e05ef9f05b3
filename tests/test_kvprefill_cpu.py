"""The prefill attention on the Q8_0 KV cache, host side (no GPU): the additive header include/gptq_gguf_kvprefill.h and its
binding, the plan, the refusals of the library and of the ops wrapper, all made before any GPU use, and generate's flags."""
import os
import re

import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")


def test_kvprefill_header_symbols_are_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_kvprefill.h")).read()
    declared = set(re.findall(r"^(?:int|size_t) (gq_[a-z0-9_]+)\s*\(", hdr, re.M))
    L = _cabi.lib()
    assert declared == set(_cabi.EXPORTS_KVPREFILL) == {"gq_attn_prefill_q8_0", "gq_attn_prefill_q8_0_plan"}
    assert all(getattr(L, name).argtypes for name in declared)
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6  # additive: the version stays


@pytest.mark.parametrize("T,G", [(1, 1), (9, 8), (64, 1), (65, 1), (512, 4), (2048, 4), (3, 200)])
def test_plan_covers_the_columns(T, G):
    from gptq_gguf_toolkit_amd import ops
    p = ops.attn_prefill_plan(T, G)
    assert p["block_cols"] >= 64 and p["turn"] % 4 == 0  # 4 rows of 68 bytes, 2 of 136: the 16-byte aligned multiples
    assert p["blocks"] * p["block_cols"] >= G * T > (p["blocks"] - 1) * p["block_cols"]


def test_library_and_ops_refuse_by_name_without_a_device():
    from gptq_gguf_toolkit_amd import _cabi, ops
    L, P = _cabi.lib(), 256

    def attn(D=64, T=70, Hq=4, S_cap=128, pos0=0, q_st=64, q=P):
        return L.gq_attn_prefill_q8_0(q, 1, 0, 64, q_st, 1, Hq, 2, T, D, P, P, S_cap, pos0, None, 1.0, P, None)
    for rc, word, kw in ((-2, "D=96", dict(D=96)), (-2, "pos0=60 + T=70 > S_cap=128", dict(pos0=60)), (-2, "Hq=5", dict(Hq=5)),
                         (-2, "multiples of 8", dict(q_st=60)), (-6, "q is NULL", dict(q=None))):
        assert attn(**kw) == rc and word in L.gq_last_error().decode(), (kw, L.gq_last_error())
    assert L.gq_attn_prefill_q8_0_plan(0, 4, None, None, None) == -2

    x = torch.zeros(1, 4, 70, 64, dtype=torch.float16)
    kc, vc = (torch.zeros(1, 2, 128, 68, dtype=torch.uint8) for _ in range(2))
    with pytest.raises(_cabi.GQError, match="D=96"):
        ops.attn_prefill_q8_0(torch.zeros(1, 4, 70, 96, dtype=torch.float16), kc, vc, 0, 1.0)
    with pytest.raises(_cabi.GQError, match=r"pos0=60 \+ T=70 > S_cap=128"):
        ops.attn_prefill_q8_0(x, kc, vc, 60, 1.0)
    with pytest.raises(_cabi.GQError, match="multiple of Hkv"):
        ops.attn_prefill_q8_0(torch.zeros(1, 5, 70, 64, dtype=torch.float16), kc, vc, 0, 1.0)
    with pytest.raises(_cabi.GQError, match="unit stride over D"):
        ops.attn_prefill_q8_0(torch.zeros(1, 4, 70, 128, dtype=torch.float16)[..., ::2], kc, vc, 0, 1.0)
    with pytest.raises(_cabi.GQError, match="kv_start must be int32"):
        ops.attn_prefill_q8_0(x, kc, vc, 0, 1.0, kv_start=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(_cabi.GQError, match="CPU"):  # good operands, 280 columns: the next thing asked for is a device
        ops.attn_prefill_q8_0(x, kc, vc, 58, 1.0, kv_start=torch.zeros(1, dtype=torch.int32))


def test_generate_prefill_flags_parse_and_default_to_one_forward_on_sdpa():
    from gptq_gguf_toolkit_amd import generate
    base = ["--model_name_or_path", "m", "--prompt_ids", "ids.pt", "--max_new_tokens", "5", "--output_file", "o.json"]
    a = generate.parse_args(base)
    assert a.prefill_chunk == 0 and a.kv_prefill == "sdpa"
    a = generate.parse_args(base + ["--kv_cache", "q8_0", "--kv_prefill", "q8_0", "--prefill_chunk", "24"])
    assert a.prefill_chunk == 24 and a.kv_prefill == "q8_0"
    with pytest.raises(SystemExit):
        generate.parse_args(base + ["--kv_prefill", "q8_0"])  # needs --kv_cache q8_0
