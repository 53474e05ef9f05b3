"""The Q8_0 KV cache, host side (no GPU): the additive header include/gptq_gguf_kvcache.h and its binding, the plan of the
split-KV attention (csrc/attn/gq_attn_plan.hpp through tests/attn_plan_dump.cpp, plain host C++) against the library's own
workspace and plan functions, and the refusals of the ops wrappers, all made before any GPU use."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
CSRC = os.path.join(ROOT, "gptq-gguf-toolkit_amd", "csrc")
LENGTHS = (1, 2, 33, 4097, 131072)


def test_kvcache_header_symbols_are_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi, ops
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_kvcache.h")).read()
    declared = set(re.findall(r"^(?:int|size_t) (gq_[a-z0-9_]+)\s*\(", hdr, re.M))
    L = _cabi.lib()
    assert declared == set(_cabi.EXPORTS_KVCACHE) and len(declared) == 4
    assert all(getattr(L, name).argtypes for name in declared)
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6  # additive: the version stays
    assert int(re.search(r"#define GQ_ATTN_DECODE_MAX_COLS (\d+)", hdr).group(1)) == ops.ATTN_DECODE_MAX_COLS == 64


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attn_plan") / "attn_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "attn_plan_dump.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("B,Hkv,cols,D", [(1, 8, 4, 128), (8, 8, 4, 128), (2, 1, 24, 64), (1, 1, 1, 64), (64, 32, 64, 128)])
def test_attn_plan_tiles_the_cache_and_is_the_librarys(dump_exe, B, Hkv, cols, D):
    from gptq_gguf_toolkit_amd import ops
    lines = subprocess.check_output([dump_exe, str(B), str(Hkv), str(cols), str(D)] + [str(s) for s in LENGTHS], text=True).splitlines()
    sub, turn, min_chunk, max_splits, max_cols = (int(v) for v in lines[0].split())
    assert max_cols == ops.ATTN_DECODE_MAX_COLS and sub % 4 == 0  # 4 rows of 68 bytes, 2 of 136: the 16-byte aligned multiples
    tiles = (cols + 15) // 16
    for S, line in zip(LENGTHS, lines[1:]):
        s, splits, chunk, ws = (int(v) for v in line.split())
        assert s == S and 1 <= splits <= max_splits
        assert chunk % sub == 0                                   # every chunk starts on the aligned multiple
        assert (splits - 1) * chunk < S <= splits * chunk         # chunks [i chunk, min(S, (i + 1) chunk)) tile [0, S), none empty
        assert splits == 1 or chunk >= min_chunk // 2             # a cache is cut only into pieces of at least a turn
        if S <= min_chunk:
            assert splits == 1
        assert ws == B * Hkv * tiles * splits * 16 * (D + 2) * 4  # the plan's need: one fp32 partial per column and chunk
        assert ops.attn_decode_workspace_bytes(S, B, Hkv, cols, D) == ws
        assert ops.attn_decode_plan(S, B, Hkv, cols) == dict(splits=splits, chunk=chunk, min_chunk=min_chunk, turn=turn)
    # a small grid is split to fill the chip, a full one is not
    big = ops.attn_decode_plan(131072, B, Hkv, cols)["splits"]
    assert big == min(max_splits, max(1, 512 // (B * Hkv * tiles)))


def _caches(B=1, Hkv=2, S_cap=8, D=64):
    return [torch.zeros(B, Hkv, S_cap, D // 32 * 34, dtype=torch.uint8) for _ in range(2)]


def test_ops_refuse_bad_operands_before_any_gpu_use():
    from gptq_gguf_toolkit_amd import _cabi, ops
    x = torch.zeros(1, 2, 3, 64, dtype=torch.float16)
    kc, vc = _caches()
    for D in (96, 256):
        bad = torch.zeros(1, 2, 3, D, dtype=torch.float16)
        with pytest.raises(_cabi.GQError, match=f"D={D}"):
            ops.kv_append_q8_0(kc, vc, bad, bad, 0)
        with pytest.raises(_cabi.GQError, match=f"D={D}"):
            ops.attn_decode_q8_0(bad, kc, vc, 0, 1.0)
    with pytest.raises(_cabi.GQError, match=r"pos0=6 \+ T=3 > S_cap=8"):
        ops.kv_append_q8_0(kc, vc, x, x, 6)
    with pytest.raises(_cabi.GQError, match=r"pos0=6 \+ T=3 > S_cap=8"):
        ops.attn_decode_q8_0(x, kc, vc, 6, 1.0)
    strided = torch.zeros(1, 2, 3, 128, dtype=torch.float16)[..., ::2]
    with pytest.raises(_cabi.GQError, match="unit stride over D"):
        ops.kv_append_q8_0(kc, vc, strided, strided, 0)
    with pytest.raises(_cabi.GQError, match="unit stride over D"):
        ops.attn_decode_q8_0(strided, kc, vc, 0, 1.0)
    with pytest.raises(_cabi.GQError, match=r"G\*T=8\*9"):  # 72 columns
        ops.attn_decode_q8_0(torch.zeros(1, 16, 9, 64, dtype=torch.float16), *_caches(S_cap=12), 0, 1.0)
    with pytest.raises(_cabi.GQError, match="S_cap % 4"):
        ops.kv_append_q8_0(*_caches(S_cap=6), x, x, 0)
    with pytest.raises(_cabi.GQError, match="CPU"):  # good operands: the next thing asked for is a device
        ops.kv_append_q8_0(kc, vc, x, x, 5)
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.attn_decode_q8_0(x, kc, vc, 5, 1.0)


def test_library_refuses_by_name_without_a_device():
    from gptq_gguf_toolkit_amd import _cabi
    L, P = _cabi.lib(), 256

    def attn(D=64, T=1, Hq=4, S_cap=8, pos0=0, ws=P, ws_bytes=1 << 20, q=P):
        return L.gq_attn_decode_q8_0(q, 1, 0, 64, 64, 1, Hq, 2, T, D, P, P, S_cap, pos0, None, 1.0, P, ws, ws_bytes, None)
    for rc, word, kw in ((-2, "D=96", dict(D=96)), (-2, "G*T=2*33", dict(T=33, S_cap=64)), (-2, "pos0=8 + T=1 > S_cap=8", dict(pos0=8)),
                         (-2, "Hq=5", dict(Hq=5)), (-3, "workspace of 16 bytes", dict(ws_bytes=16)), (-6, "q is NULL", dict(q=None))):
        assert attn(**kw) == rc and word in L.gq_last_error().decode(), (kw, L.gq_last_error())
    assert L.gq_kv_append_q8_0(P, P, 1, 0, 64, 60, 1, 2, 1, 64, P, P, 8, 0, None) == -2 and b"multiples of 8" in L.gq_last_error()
    assert L.gq_kv_append_q8_0(P, P, 0, 0, 64, 64, 1, 2, 1, 64, P, P, 8, 0, None) == -1  # fp32 rows: no such path


def test_generate_kv_cache_flag_parses_and_defaults_to_hf():
    from gptq_gguf_toolkit_amd import generate
    base = ["--model_name_or_path", "m", "--prompt_ids", "ids.pt", "--max_new_tokens", "5", "--output_file", "o.json"]
    assert generate.parse_args(base).kv_cache == "hf"
    assert generate.parse_args(base + ["--kv_cache", "q8_0"]).kv_cache == "q8_0"
    with pytest.raises(SystemExit):
        generate.parse_args(base + ["--kv_cache", "q4_0"])
