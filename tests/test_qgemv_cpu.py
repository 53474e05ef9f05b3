"""The packed-weight decode, host side (no GPU): the additive header include/gptq_gguf_qgemv.h and its binding, every refusal
of gq_gemv_packed -- made before the first HIP call, so host pointers do --, the routing of PackedLinear between the GEMV and
the tile kernel, generate's flags, and greedy() against one full forward on the fp32 CPU tiny Llama (the cache plumbing)."""
import ctypes
import os
import re
import sys

import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

P = 256  # any 16-byte aligned address, never dereferenced
F16, BF16 = 1, 2
BAD_TYPE, BAD_SHAPE, NULL = -1, -2, -6


def _msg(L):
    return L.gq_last_error().decode()


def test_qgemv_header_symbol_is_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi, ops
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_qgemv.h")).read()
    declared = set(re.findall(r"^int (gq_[a-z0-9_]+)\s*\(", hdr, re.M))
    L = _cabi.lib()
    assert declared == set(_cabi.EXPORTS_QGEMV) == {"gq_gemv_packed"}
    assert hasattr(ctypes.CDLL(_cabi.SO_PATH), "gq_gemv_packed") and len(L.gq_gemv_packed.argtypes) == 10
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6 and len(_cabi.EXPORTS) == 48  # additive: the version stays
    assert _cabi.EXPORTS_QGEMM == ("gq_linear_packed",)
    assert '#include "gptq_gguf_qgemm.h"' in hdr
    for word in ("GQ_GEMV_MAX_T", "Deterministic", "summation order"):
        assert word in hdr, word
    assert int(re.search(r"#define GQ_GEMV_MAX_T (\d+)", hdr).group(1)) == _cabi.GEMV_MAX_T == ops.GEMV_MAX_T == 16
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "gptq_gguf_qgemv.h" in text and "gq_gemv_packed" in text, doc
    assert "(48 symbols)" in open(os.path.join(ROOT, "README.md")).read()


def test_gemv_packed_refusals_need_no_device():
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()

    def call(q_type=12, blocks=P, row_src=None, R=4, C=256, x=P, T=3, x_dtype=F16, y=P):
        return L.gq_gemv_packed(q_type, blocks, row_src, R, C, x, T, x_dtype, y, None)

    def refused(status, word, **kw):
        rc = call(**kw)
        assert rc == status and word in _msg(L) and "gq_gemv_packed" in _msg(L), (kw, rc, _msg(L))

    refused(BAD_SHAPE, "C=128", C=128)
    refused(BAD_SHAPE, "C=288", q_type=8, C=288)          # Q8_0 too: a multiple of 32 is not enough here
    refused(BAD_SHAPE, "C=0", C=0)
    refused(BAD_SHAPE, "R=0", R=0)
    refused(BAD_SHAPE, "T=0", T=0)
    refused(BAD_SHAPE, "T=17", T=17)
    refused(BAD_SHAPE, "T=-1", T=-1)
    refused(BAD_SHAPE, "T=2147483647", T=(1 << 31) - 1)
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
    # the order of the checks is gq_linear_packed's: type, NULL, R, T, C, alignments
    refused(BAD_TYPE, "q_type 3", q_type=3, T=17, x=None)
    refused(NULL, "x is NULL", x=None, T=17)
    refused(BAD_SHAPE, "R=0", R=0, T=17)
    refused(BAD_SHAPE, "T=17", T=17, C=128, y=P + 2)
    # T = 16 is the last T that passes the T rule: the refusal is the NEXT check's, and T = 16 with good arguments is left to
    # the GPU file (it launches)
    refused(BAD_SHAPE, "y not 16-byte aligned", T=16, y=P + 2)
    refused(BAD_SHAPE, "y not 16-byte aligned", T=1, y=P + 2)


def test_gemv_packed_names_the_earlier_of_two_faults():
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
        rc = L.gq_gemv_packed(args["q_type"], args["blocks"], args["row_src"], args["R"], args["C"], args["x"], args["T"],
                              args["x_dtype"], args["y"], None)
        assert rc == status and _msg(L).startswith("gq_gemv_packed: ") and word in _msg(L), (kw, rc, _msg(L))


def test_ops_gemv_packed_refuses_cpu_tensors():
    from gptq_gguf_toolkit_amd import _cabi, ops
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.gemv_packed(12, torch.zeros(4, 144, dtype=torch.uint8), torch.zeros(3, 256, dtype=torch.float16))


def test_packed_linear_routes_few_tokens_to_the_gemv(monkeypatch):
    from gptq_gguf_toolkit_amd import ops
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    C, R = 256, 8
    calls = []

    def recorder(name):
        def fn(q_type, blocks, x, row_src=None):
            assert x.is_contiguous() and x.shape[-1] == C
            calls.append((name, tuple(x.shape)))
            return torch.zeros(*x.shape[:-1], R, dtype=x.dtype)
        return fn

    monkeypatch.setattr(ops, "gemv_packed", recorder("gemv"))
    monkeypatch.setattr(ops, "linear_packed", recorder("gemm"))
    assert PackedLinear.gemv_max_t == ops.GEMV_MAX_T == 16
    lin = PackedLinear(C, R)
    lin.set_level(torch.zeros(R, 144, dtype=torch.uint8), 12)
    shapes = [(1, C), (16, C), (2, 8, C), (17, C), (2, 9, C)]
    for s in shapes:
        assert lin(torch.zeros(*s, dtype=torch.float16)).shape == (*s[:-1], R)
    assert calls == [("gemv", shapes[0]), ("gemv", shapes[1]), ("gemv", shapes[2]), ("gemm", shapes[3]), ("gemm", shapes[4])]

    del calls[:]
    lin.gemv_max_t = 4  # an instance may override the class attribute
    lin(torch.zeros(4, C, dtype=torch.float16)), lin(torch.zeros(5, C, dtype=torch.float16))
    assert [c[0] for c in calls] == ["gemv", "gemm"] and PackedLinear.gemv_max_t == 16

    del calls[:]
    lin.gemv_max_t = 0  # the routing off: everything is the tile kernel's
    for s in shapes:
        lin(torch.zeros(*s, dtype=torch.float16))
    assert calls == [("gemm", s) for s in shapes]

    del calls[:]
    dense = PackedLinear(C, R)
    dense.set_level(torch.ones(R, C, dtype=torch.float16), None)  # a dense level: F.linear on the stored tensor
    x = torch.ones(1, C, dtype=torch.float16)
    assert torch.equal(dense(x), torch.full((1, R), float(C), dtype=torch.float16)) and calls == []


def test_generate_flags_parse_and_default():
    from gptq_gguf_toolkit_amd import generate
    base = ["--model_name_or_path", "m", "--prompt_ids", "ids.pt", "--max_new_tokens", "5", "--output_file", "o.json"]
    a = generate.parse_args(base)
    assert (a.gguf, a.packed, a.quant_weights_path, a.quant_config_path, a.quant_default_level) == (None, False, None, None, 0)
    assert (a.dtype, a.attn_implementation, a.tokenizer_name, a.max_new_tokens) == ("float16", None, None, 5)
    a = generate.parse_args(base + ["--gguf", "f.gguf", "--packed", "--dtype", "bfloat16", "--attn_implementation", "eager",
                                    "--tokenizer_name", "tok"])
    assert a.packed and a.gguf == "f.gguf" and a.dtype == "bfloat16" and a.attn_implementation == "eager" and a.tokenizer_name == "tok"
    a = generate.parse_args(base + ["--quant_weights_path", "db", "--quant_config_path", "cfg"])
    assert (a.quant_weights_path, a.quant_config_path) == ("db", "cfg")
    for bad in (["--packed"], ["--gguf", "f", "--quant_weights_path", "db"], ["--quant_config_path", "cfg"]):
        with pytest.raises(SystemExit):
            generate.parse_args(base + bad)
    with pytest.raises(SystemExit):
        generate.parse_args(base[:4] + ["--max_new_tokens", "0"] + base[6:])


def test_greedy_with_the_cache_equals_one_full_forward():
    """48 prompt tokens, 16 new ones, samples 0 and 1: the ids greedy() produced must be the argmax of ONE full forward over
    the produced sequence at positions 47 .. 62, and the logits it returns must be that forward's rows up to fp32 rounding.
    The smallest top-2 margin of these two runs is 0.005 at max |logit| 1.2; the cached and the full forward are the same
    fp32 arithmetic on differently shaped matrices, so they differ by about 1e-6."""
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd.generate import greedy
    model = tiny_llama().eval()
    calib = tiny_calib(n=3, L=64, seed=29)
    for sample in (0, 1):
        prompt = calib[sample][:, :48]
        ids, logits = greedy(model, prompt, 16, return_logits=True)
        assert ids.shape == (1, 64) and logits.shape == (1, 16, 512) and torch.equal(ids[:, :48], prompt)
        assert torch.equal(ids[:, 48:], logits.argmax(-1))
        assert torch.equal(greedy(model, prompt, 16), ids)
        with torch.no_grad():
            full = model(ids).logits[:, 47:63]
        diff = float((full - logits).abs().max())
        top2 = full.topk(2, -1).values
        print(f"sample {sample}: cached against full forward max |difference| {diff:.3e}, smallest top-2 margin "
              f"{float((top2[..., 0] - top2[..., 1]).min()):.3e}, max |logit| {float(full.abs().max()):.3f}")
        assert torch.equal(ids[:, 48:], full.argmax(-1))
        assert diff <= 1e-4
    with pytest.raises(ValueError, match="max_new_tokens"):
        greedy(model, calib[0], 0)
