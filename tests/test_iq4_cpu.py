"""IQ4_NL and IQ4_XS, host side (no GPU): the scalar restatement of the two decoders (tests/iq4_spec.py) against the header's
anchors and against the torch expression of its contract, the fixtures of tests/test_gpu_iq4.py, the additive header
include/gptq_gguf_iq4.h and its bindings, every refusal of the entry points that take the two types -- made before the first
HIP call, so host pointers do --, the entry points that keep refusing them, and the writer, the level database and the
stitcher passing their bytes through."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import iq4_spec as S
from conftest import ROOT
from gguf_spec_reader import read_kv

torch = pytest.importorskip("torch")

NL, XS = S.NL, S.XS
P = 256  # any 16-byte aligned address, never dereferenced
BAD_TYPE, BAD_SHAPE, NULL = -1, -2, -6


def _msg(L):
    return L.gq_last_error().decode()


# ------------------------------------------------------------------------------------------------ 1: the restatement
def test_the_two_anchors():
    y = S.decode_iq4_nl(S.nl_block(0x3800, [0x80] + [0] * 15), 32)
    assert y[0] == -63.5 and y[16] == 0.5
    qs = [0] * 128
    qs[0], qs[16] = 0xF0, 0x08
    blk = S.xs_block(0x3C00, 0x0003, [0x21, 0, 0, 0], qs)
    assert [S.xs_scale(blk, 0), S.xs_scale(blk, 1)] == [49, 2]
    y = S.decode_iq4_xs(blk, 256)
    assert [y[0], y[16], y[32], y[48]] == [-2159.0, 1921.0, -30.0, 3810.0]


def torch_expression(t, blocks):
    """(d.float() * (ls - 32).float() * kv.float()) of the contract, vectorised: fp32 [R, C]."""
    bs, ts = S.GEOMETRY[t]
    b = torch.from_numpy(np.ascontiguousarray(blocks)).reshape(-1, ts)
    kv = torch.tensor(S.KV, dtype=torch.int32)
    d = b[:, :2].contiguous().view(torch.float16).float()  # [nb, 1]
    if t == NL:
        qs = b[:, 2:].int()
        w = d.unsqueeze(-1) * torch.stack([kv[qs & 15], kv[qs >> 4]], 1).float()                # [nb, 2, 16]
    else:
        sh = b[:, 2].int() | (b[:, 3].int() << 8)
        ib = torch.arange(8)
        ls = ((b[:, 4:8].int()[:, ib // 2] >> (4 * (ib % 2))) & 15) | (((sh[:, None] >> (2 * ib)) & 3) << 4)
        qs = b[:, 8:].int().reshape(-1, 8, 16)
        w = (d * (ls - 32).float())[:, :, None, None] * torch.stack([kv[qs & 15], kv[qs >> 4]], 2).float()  # [nb, 8, 2, 16]
    return w.reshape(blocks.shape[0], -1)


@pytest.mark.parametrize("t,R,C", S.DEQUANT_CASES, ids=[f"{S.NAME[c[0]]}-{c[1]}x{c[2]}" for c in S.DEQUANT_CASES])
def test_spec_equals_the_torch_expression_of_the_contract(t, R, C):
    blocks = S.dequant_fixture(t, R, C)
    want, got = torch_expression(t, blocks), torch.from_numpy(S.decode(t, blocks))
    assert got.shape == (R, C) and bool(torch.isfinite(want).all())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    for dt in (torch.float16, torch.bfloat16):  # the cast is torch's in both: checked so that the GPU tests may rely on it
        assert torch.equal(got.to(dt).view(torch.int16), want.to(dt).view(torch.int16))


def test_a_non_finite_d_propagates():
    for t, R, C in ((XS, 5, 512), (NL, 5, 96)):
        blocks = S.with_inf_block(t, S.dequant_fixture(t, R, C))
        got, want = S.decode(t, blocks), torch_expression(t, blocks).numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])
        bs = S.GEOMETRY[t][0]
        blk = got.reshape(-1)[bs:2 * bs]  # block 1
        if t == XS:
            assert np.isnan(blk[:32]).all() and np.isinf(blk[32:64]).all() and not np.isfinite(blk).any()  # ls 32, 33
        else:
            assert np.isinf(blk).all()  # kv is never 0
        assert np.isfinite(np.delete(got.reshape(-1, bs), 1, axis=0)).all()


def test_fixtures_cover_every_scale_and_code_and_every_kind_of_d():
    for cases, fixture in ((S.DEQUANT_CASES, S.dequant_fixture), (S.GEMM_CASES + S.EXPERT_CASES, S.gemm_fixture)):
        seen_ls, seen_codes = {XS: set(), NL: set()}, {XS: set(), NL: set()}
        for t, R, C in cases:
            ls, codes = S.scales_and_codes(t, fixture(t, R, C))
            seen_ls[t] |= ls
            seen_codes[t] |= codes
        assert seen_ls[XS] == set(range(64)) and seen_codes[XS] == seen_codes[NL] == set(range(16))
    for t, R, C in S.DEQUANT_CASES:
        d = S.dequant_fixture(t, R, C).reshape(-1, S.GEOMETRY[t][1])[:, :2].copy().view(np.float16).ravel()
        assert np.isfinite(d).all() and (d > 0).any() and (d < 0).any()
        assert ((d != 0) & (np.abs(d) < np.float16(6.104e-5))).any()  # fp16 subnormals
    for t, R, C in S.GEMM_CASES + S.EXPERT_CASES:
        blocks = S.gemm_fixture(t, R, C)
        d = np.abs(blocks.reshape(-1, S.GEOMETRY[t][1])[:, :2].copy().view(np.float16).astype(np.float32).ravel())
        assert d.min() >= 2.0 ** -10 and d.max() < 2.0 ** -1
        w = torch.from_numpy(S.decode(t, blocks))
        nz = w[w != 0].abs()
        assert bool(torch.isfinite(w).all()) and float(nz.min()) >= 2.0 ** -10 and float(w.abs().max()) <= 2032.0
        for dt in (torch.float16, torch.bfloat16):  # no 16-bit subnormal, no overflow: the GEMM comparisons exclude nothing
            wd = w.to(dt)
            assert bool(torch.isfinite(wd).all()) and not bool(((wd != 0) & (wd.float().abs() < torch.finfo(dt).tiny)).any())


# ------------------------------------------------------------------------------------------------ 2: header and bindings
def test_header_defines_equal_the_bindings_and_declare_no_symbol():
    from gptq_gguf_toolkit_amd import _cabi, ops
    from gptq_gguf_toolkit_amd.gguf_writer import GGML_QUANT_SIZES, PACKED_TYPES, GGMLType
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_iq4.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (GQ_IQ4_\w+) (\d+)", hdr)}
    assert defs == {"GQ_IQ4_NL": 20, "GQ_IQ4_XS": 23}
    assert (_cabi.IQ4_NL, _cabi.IQ4_XS) == (int(GGMLType.IQ4_NL), int(GGMLType.IQ4_XS)) == (20, 23) == (NL, XS)
    assert not re.findall(r"^int (gq_[a-z0-9_]+)\s*\(", hdr, re.M)  # no new symbol
    assert _cabi.lib().gq_abi_version() == _cabi.ABI_VERSION == 6
    table = [int(v) for v in re.search(r"kv\[16\] = \{([^}]*)\}", hdr).group(1).split(",")]
    assert tuple(table) == S.KV
    assert GGML_QUANT_SIZES[GGMLType.IQ4_NL] == (32, 18) and GGML_QUANT_SIZES[GGMLType.IQ4_XS] == (256, 136)
    assert ops.block_geometry(20) == (32, 18) and ops.block_geometry(23) == (256, 136)
    assert ops.block_geometry(8) == (32, 34) and ops.block_geometry(12) == (256, 144)
    assert {20, 23} <= set(PACKED_TYPES)
    assert sorted(PACKED_TYPES) == [8, 10, 11, 12, 13, 14, 20, 23]
    for t in PACKED_TYPES:
        assert ops.block_geometry(t) == GGML_QUANT_SIZES[t]
    for t in (9, 15):
        with pytest.raises(_cabi.GQError, match=f"q_type {t}"):
            ops.block_geometry(t)
    assert "gptq_gguf_iq4.h" in open(os.path.join(ROOT, "README.md")).read()
    assert "gptq_gguf_iq4.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ------------------------------------------------------------------------------------------------ 3: refusals
def test_dequantize_blocks_takes_the_two_types_and_checks_their_rules():
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()
    deq = L.gq_dequantize_blocks
    assert deq(NL, P, 4, 48, None, P, 1, None) == BAD_SHAPE and "C=48" in _msg(L) and "32" in _msg(L)
    assert deq(XS, P, 4, 96, None, P, 1, None) == BAD_SHAPE and "C=96" in _msg(L) and "256" in _msg(L)
    assert deq(XS, P, 4, 288, None, P, 1, None) == BAD_SHAPE
    assert deq(NL, P, 0, 96, None, P, 1, None) == BAD_SHAPE and deq(XS, P, 0, 256, None, P, 1, None) == BAD_SHAPE
    assert deq(NL, P + 1, 4, 96, None, P, 1, None) == BAD_SHAPE and "2-byte aligned" in _msg(L)
    for off in (2, 4, 12):
        assert deq(XS, P + off, 4, 256, None, P, 1, None) == BAD_SHAPE and "8-byte aligned" in _msg(L)
    assert deq(NL, P + 2, 4, 96, None, P + 8, 1, None) == BAD_SHAPE and "16-byte aligned" in _msg(L)
    assert deq(XS, P + 8, 4, 256, None, P + 8, 2, None) == BAD_SHAPE and "16-byte aligned" in _msg(L)
    for t, C in ((NL, 96), (XS, 256)):
        assert deq(t, None, 4, C, None, P, 1, None) == NULL and deq(t, P, 4, C, None, None, 1, None) == NULL
        assert deq(t, P, 4, C, None, P, 5, None) == BAD_TYPE and "out_dtype 5" in _msg(L)
    for q_type in (3, 9, 15, 16, 21, 22):
        assert deq(q_type, P, 4, 256, None, P, 1, None) == BAD_TYPE and f"q_type {q_type}" in _msg(L)


def test_level_switch_takes_the_two_kinds_and_checks_their_rules():
    from gptq_gguf_toolkit_amd import _cabi
    L, J = _cabi.lib(), _cabi.SwitchJob

    def refused(jobs, status, *words):
        rc = L.gq_level_switch((J * len(jobs))(*jobs), len(jobs), None)
        assert rc == status and all(w in _msg(L) for w in words), (rc, _msg(L))

    ok = J(P, P, None, 4, 256, 12, 1)
    refused([ok, J(P, P, None, 4, 48, NL, 1)], BAD_SHAPE, "job 1", "C=48", "32")
    refused([ok, J(P, P, None, 4, 96, XS, 1)], BAD_SHAPE, "job 1", "C=96", "256")
    refused([J(P + 1, P, None, 4, 96, NL, 1)], BAD_SHAPE, "job 0", "src not 2-byte aligned")
    refused([J(P + 4, P, None, 4, 256, XS, 1)], BAD_SHAPE, "job 0", "src not 8-byte aligned")
    refused([J(P + 2, P, None, 4, 256, XS, 2)], BAD_SHAPE, "job 0", "src not 8-byte aligned")
    refused([J(P + 2, P + 8, None, 4, 96, NL, 1)], BAD_SHAPE, "job 0", "dst not 16-byte aligned")  # src 2-byte aligned is enough
    refused([J(P + 8, P + 8, None, 4, 256, XS, 0)], BAD_SHAPE, "job 0", "dst not 16-byte aligned")  # src 8-byte aligned is enough
    for kind, C in ((NL, 96), (XS, 256)):
        refused([J(P, P, None, 0, C, kind, 1)], BAD_SHAPE, "job 0", "R=0")
        refused([J(None, P, None, 4, C, kind, 1)], NULL, "job 0", "src is NULL")
        refused([J(P, P, None, 4, C, kind, 3)], BAD_TYPE, "job 0", "out_dtype 3")
        refused([J(P, P, P + 2, 4, C, kind, 1)], BAD_SHAPE, "job 0", "row_src")
        refused([J(P, P, None, 1 << 50, C, kind, 1)], BAD_SHAPE, "job 0", "more than one launch")
    for kind in (3, 9, 15, 16, 21, 22):  # the neighbours stay unknown
        refused([J(P, P, None, 4, 256, kind, 1)], BAD_TYPE, "job 0", f"kind {kind}")


def test_the_packed_forward_takes_the_two_types_and_checks_their_rules():
    """Each call differs from a good one in ONE argument, so the refusal is that argument's; C = 288 for IQ4_NL is the rule
    that the packed forward needs whole superblocks of every type."""
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()
    calls = {
        "gq_linear_packed": lambda t, b, C: L.gq_linear_packed(t, b, None, 4, C, P, 3, 1, P, None),
        "gq_gemv_packed": lambda t, b, C: L.gq_gemv_packed(t, b, None, 4, C, P, 3, 1, P, None),
        "gq_gemv_packed_experts": lambda t, b, C: L.gq_gemv_packed_experts(t, b, 2, 4, C, P, 3, P, 3, 1, 1, P, None),
        "gq_linear_packed_experts": lambda t, b, C: L.gq_linear_packed_experts(t, b, 2, 4, C, P, 3, 1, P, P, 3, 1, P, None),
    }
    for name, call in calls.items():
        for t in (NL, XS):
            assert call(t, P, 128) == BAD_SHAPE and name in _msg(L) and "C=128" in _msg(L)  # past the type check
            assert call(t, None, 256) == NULL and "blocks is NULL" in _msg(L)
        assert call(NL, P, 288) == BAD_SHAPE and "C=288" in _msg(L)       # C % 32 == 0 is not enough here
        assert call(NL, P + 1, 256) == BAD_SHAPE and "blocks not 2-byte aligned" in _msg(L)
        for off in (2, 4, 12):
            assert call(XS, P + off, 256) == BAD_SHAPE and "blocks not 8-byte aligned" in _msg(L)
        assert call(12, P + 8, 256) == BAD_SHAPE and "blocks not 16-byte aligned" in _msg(L)  # (Q4_K keeps its own)
        for t in (3, 9, 15, 16, 21, 22):
            assert call(t, P, 256) == BAD_TYPE and f"q_type {t}" in _msg(L)


def test_every_other_entry_point_keeps_refusing_types_20_and_23():
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()
    s = _cabi.Search(-1.0, 0.1, 20, 0, 100, 0.8)
    for t in (NL, XS):
        assert L.gq_pack(t, P, P, P, P, P, 4, 256, P, None) == BAD_TYPE and f"q_type {t}" in _msg(L)
        assert L.gq_unpack(t, P, 4, 256, P, P, P, P, P, None) == BAD_TYPE and f"q_type {t}" in _msg(L)
        assert L.gq_type_info(t, ctypes.byref(_cabi.TypeInfo())) == BAD_TYPE
        assert L.gq_rtn_quantize(P, 0, 4, 256, t, ctypes.byref(s), P, P, P, P, P, None) == BAD_TYPE
        bands = (_cabi.Band * 1)(_cabi.Band(64, t))
        outs = (ctypes.c_void_p * 1)(P)
        assert L.gq_pack_bands(P, P, P, P, P, 64, 256, bands, 1, outs, None, None) == BAD_TYPE
        assert L.gq_gptq_quantize_bands(P, P, 64, 256, bands, 1, 128, ctypes.byref(s), P, P, P, P, P, P, 1 << 30, None) == BAD_TYPE
        assert L.gq_quantize_q8_0(P, t, 4, 64, None, P, None) == BAD_TYPE  # (no input dtype either)


def test_ops_and_modules_size_the_two_types():
    from gptq_gguf_toolkit_amd import _cabi, ops
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.dequantize_blocks(XS, torch.zeros(4, 136, dtype=torch.uint8))
    m = PackedLinear(512, 8)
    m.set_level(torch.zeros(8 * 2 * 136, dtype=torch.uint8), XS)
    m.set_level(torch.zeros(8 * 16 * 18, dtype=torch.uint8), NL)
    assert m.q_type == NL
    with pytest.raises(_cabi.GQError, match="must be 2176 uint8"):
        m.set_level(torch.zeros(8 * 2 * 144, dtype=torch.uint8), XS)
    with pytest.raises(_cabi.GQError, match=r"in_features % 256 == 0"):  # IQ4_NL rows of 96 values: a valid tensor, never packed
        PackedLinear(96, 8).set_level(torch.zeros(8 * 3 * 18, dtype=torch.uint8), NL)


# ------------------------------------------------------------------------------------------------ 4: files
def read_tensors(path):
    """(key/value data, [(name, logical shape, ggml type, payload)] in file order), from the GGUF v3 specification: the
    key/value data through tests/gguf_spec_reader.py; then n_tensors x {string name, u32 n_dims, u64 dims[n_dims] (innermost
    first), u32 type, u64 offset}; the data section starts at the next multiple of 32 and every payload is padded to 32."""
    buf = open(path, "rb").read()
    kv, _, n_tensors = read_kv(path)
    scalar = {0: 1, 1: 1, 2: 2, 3: 2, 4: 4, 5: 4, 6: 4, 7: 1, 10: 8, 11: 8, 12: 8}
    pos = 24

    def skip_value(t):
        nonlocal pos
        if t == 8:
            pos += 8 + struct.unpack_from("<Q", buf, pos)[0]
        elif t == 9:
            et, cnt = struct.unpack_from("<IQ", buf, pos)
            pos += 12
            for _ in range(cnt):
                skip_value(et)
        else:
            pos += scalar[t]

    for _ in range(len(kv)):
        skip_value(8)
        t = struct.unpack_from("<I", buf, pos)[0]
        pos += 4
        skip_value(t)
    infos = []
    for _ in range(n_tensors):
        n = struct.unpack_from("<Q", buf, pos)[0]
        name = buf[pos + 8:pos + 8 + n].decode()
        pos += 8 + n
        nd = struct.unpack_from("<I", buf, pos)[0]
        dims = struct.unpack_from(f"<{nd}Q", buf, pos + 4)
        gt, off = struct.unpack_from("<IQ", buf, pos + 4 + 8 * nd)
        pos += 4 + 8 * nd + 12
        infos.append((name, tuple(reversed(dims)), gt, off))
    data0 = (pos + 31) // 32 * 32
    sizes = {0: (1, 4), 1: (1, 2), 12: (256, 144), NL: S.GEOMETRY[NL], XS: S.GEOMETRY[XS]}
    out = []
    for name, shape, gt, off in infos:
        bs, ts = sizes[gt]
        nbytes = int(np.prod(shape)) // bs * ts
        assert off % 32 == 0 and data0 + off + nbytes <= len(buf), name
        out.append((name, shape, gt, buf[data0 + off:data0 + off + nbytes]))
    assert len(buf) % 32 == 0
    return kv, out


XS_TENSORS = ("blk.0.attn_q.weight", "blk.0.attn_k.weight", "blk.0.attn_v.weight", "blk.0.attn_output.weight")


@pytest.fixture(scope="module")
def database(tmp_path_factory):
    """A tiny --gguf-layers database from the level writer: four attention tensors [4, 256] with an IQ4_XS level each (attn_q
    also a Q4_K one), ffn_down [4, 96] (rows no multiple of 256) with an IQ4_NL level, two plain tensors."""
    from gptq_gguf_toolkit_amd import level_db
    from gptq_gguf_toolkit_amd.gguf_writer import GGUFWriter, kv_records
    tmp = tmp_path_factory.mktemp("iq4db")
    rng = np.random.default_rng(5)
    w = GGUFWriter(str(tmp / "unused.gguf"), "llama")
    w.add_uint32("llama.block_count", 1)
    payload = {("token_embd.weight", 1): rng.standard_normal((8, 256)).astype(np.float16),
               ("blk.0.attn_q.weight", 12): rng.integers(0, 256, (4, 144), dtype=np.uint8)}
    for i, name in enumerate(XS_TENSORS):
        payload[(name, XS)] = S.blocks_with_d(XS, 4, 256, seed=50 + i)
    payload[("blk.0.ffn_down.weight", NL)] = S.dequant_fixture(NL, 4, 96)
    payload[("output_norm.weight", 0)] = rng.standard_normal(256).astype(np.float32)
    shapes = {"token_embd.weight": (8, 256), **{n: (4, 256) for n in XS_TENSORS}, "blk.0.ffn_down.weight": (4, 96),
              "output_norm.weight": (256,)}
    with level_db.LevelDbWriter(str(tmp / "db")) as wr:
        for (name, gt), data in payload.items():
            wr.add_level(name, shapes[name], gt, data)
        wr.set_metadata(kv_records(w.kv))
        wr.set_order(list(shapes))
    return tmp / "db", payload, shapes


def test_level_database_names_and_sizes_the_two_types(database):
    from gptq_gguf_toolkit_amd import level_db
    db, payload, _ = database
    assert level_db.TYPE_NAMES[NL] == "IQ4_NL" and level_db.TYPE_NAMES[XS] == "IQ4_XS"
    assert level_db.EXACT_BITS["IQ4_NL"] == 4.56 and level_db.EXACT_BITS["IQ4_XS"] == 4.25  # the reference's table widths
    avail = level_db.scan_available_bitwidths(str(db))
    assert avail["blk.0.attn_q.weight"] == [(4.25, "4.25-IQ4_XS.pth"), (4.5, "4.5-Q4_K.pth")]
    assert avail["blk.0.ffn_down.weight"] == [(4.56, "4.56-IQ4_NL.pth")]
    for name, fname, t in (("blk.0.attn_q.weight", "4.25-IQ4_XS.pth", XS), ("blk.0.ffn_down.weight", "4.56-IQ4_NL.pth", NL)):
        rec = level_db.read_sidecar(str(db / name / fname))
        assert rec.ggml_type == t and rec.quantization == S.NAME[t] and rec.np_shape == list(payload[(name, t)].shape)
        assert level_db.check_level_size(rec) == payload[(name, t)].nbytes
        assert np.array_equal(level_db.read_level_raw(rec).reshape(rec.np_shape), payload[(name, t)])
    with pytest.raises(ValueError, match="no multiple of the block of 256"):
        with level_db.LevelDbWriter(str(db) + "2") as wr:
            wr.register("blk.0.ffn_down.weight", (4, 96), XS)
    with pytest.raises(ValueError, match="cannot be a level"):
        with level_db.LevelDbWriter(str(db) + "3") as wr:
            wr.register("blk.0.ffn_down.weight", (4, 256), 16)  # IQ2_XXS


CONFIG = ("token_embd.weight: 16 (16-F16.pth)\n" + "".join(f"{n}: 4.25 (4.25-IQ4_XS.pth)\n" for n in XS_TENSORS) +
          "blk.0.ffn_down.weight: 4.56 (4.56-IQ4_NL.pth)\noutput_norm.weight: 32 (32-F32.pth)\n")


def test_stitcher_writes_both_types_and_still_refuses_iq2_xxs(database, tmp_path):
    import json
    import shutil
    from gptq_gguf_toolkit_amd import gguf_stitcher
    from gptq_gguf_toolkit_amd.gguf_stitcher import GGUFStitcher
    db, payload, shapes = database
    assert gguf_stitcher.LLAMA_FTYPE["IQ4_NL"] == 25 and gguf_stitcher.LLAMA_FTYPE["IQ4_XS"] == 30
    assert gguf_stitcher.WRITABLE["IQ4_NL"] == NL and gguf_stitcher.WRITABLE["IQ4_XS"] == XS and "IQ2_XXS" not in gguf_stitcher.WRITABLE
    (tmp_path / "c.txt").write_text(CONFIG)
    st = GGUFStitcher(str(db), str(tmp_path / "c.txt"), str(tmp_path / "out.gguf"), quiet=True, llama_ftype=True)
    planned = {p.name: p for p in st.plan()}
    assert planned["blk.0.attn_q.weight"].type_name == "IQ4_XS" and planned["blk.0.attn_q.weight"].ggml_type == XS
    assert planned["blk.0.ffn_down.weight"].type_name == "IQ4_NL" and planned["blk.0.ffn_down.weight"].nbytes == 4 * 3 * 18
    assert st._calculate_file_type() == 30  # four of seven tensors are IQ4_XS: LLAMA_FTYPE_MOSTLY_IQ4_XS
    st.stitch_model()
    kv, got = read_tensors(str(tmp_path / "out.gguf"))
    want = [("token_embd.weight", 1)] + [(n, XS) for n in XS_TENSORS] + [("blk.0.ffn_down.weight", NL), ("output_norm.weight", 0)]
    assert [(n, s, t) for n, s, t, _ in got] == [(n, shapes[n], t) for n, t in want]
    for (name, _, t, raw), key in zip(got, want):
        assert raw == payload[key].tobytes(), name
    assert kv["llama.block_count"] == 1 and kv["general.file_type"] == 30
    # IQ2_XXS stays refused by name, and nothing is written
    db2 = tmp_path / "db2"
    shutil.copytree(db, db2)
    d = db2 / "blk.9.extra.weight"
    d.mkdir()
    (d / "2.06-IQ2_XXS.pth").write_bytes(bytes(66))
    (d / "2.06-IQ2_XXS-metadata.json").write_text(json.dumps({"tensor_info": {
        "name": d.name, "type": 16, "quantization": "IQ2_XXS", "shape": [256, 1], "np_dtype": "uint8", "np_shape": [1, 66]}}))
    with pytest.raises(gguf_stitcher.StitchError, match="IQ2_XXS"):
        GGUFStitcher(str(db2), str(tmp_path / "c.txt"), str(tmp_path / "o2.gguf"), quiet=True).stitch_model()
    assert not (tmp_path / "o2.gguf").exists()


def test_writer_and_parser_pass_the_payload_through(tmp_path):
    from gptq_gguf_toolkit_amd.gguf_writer import GGMLType, GGUFWriter, parse_gguf, quant_shape_from_byte_shape
    assert quant_shape_from_byte_shape((4, 3 * 18), GGMLType.IQ4_NL) == (4, 96)
    assert quant_shape_from_byte_shape((2, 4, 2 * 136), GGMLType.IQ4_XS) == (2, 4, 512)
    w = GGUFWriter(str(tmp_path / "w.gguf"), "llama")
    a, b = S.dequant_fixture(NL, 4, 96), S.dequant_fixture(XS, 4, 256)
    w.add_tensor("token_embd.weight", a, raw_dtype=GGMLType.IQ4_NL)
    w.add_tensor("blk.0.attn_q.weight", b, raw_dtype=GGMLType.IQ4_XS)
    w.write()
    _, got = read_tensors(str(tmp_path / "w.gguf"))
    assert [(n, s, t) for n, s, t, _ in got] == [("token_embd.weight", (4, 96), NL), ("blk.0.attn_q.weight", (4, 256), XS)]
    assert got[0][3] == a.tobytes() and got[1][3] == b.tobytes()
    _, tensors, buf = parse_gguf(str(tmp_path / "w.gguf"))
    assert [(n, s, t, nb) for n, s, t, _, nb in tensors] == [("token_embd.weight", (4, 96), NL, 216), ("blk.0.attn_q.weight", (4, 256), XS, 544)]
    assert all(off % 8 == 0 for _, _, _, off, _ in tensors)  # (32-byte tensor alignment: an IQ4_XS block is 8-byte aligned)


def test_loader_keeps_only_whole_superblock_rows_packed(tmp_path):
    """An IQ4_NL tensor with rows of 96 values is a valid file tensor; it is not among the tensors kept packed (it loads
    dense), one with rows of 256 is."""
    import gguf_spec_writer as W
    import torch.nn as nn
    from gptq_gguf_toolkit_amd import gguf_loader

    class Mlp(nn.Module):
        def __init__(self):
            super().__init__()
            self.down_proj, self.up_proj = nn.Linear(96, 8, bias=False), nn.Linear(256, 8, bias=False)

    class Layer(nn.Module):
        def __init__(self):
            super().__init__()
            self.mlp = Mlp()

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.model = nn.Module()
            self.model.layers = nn.ModuleList([Layer()])

    tensors = [("blk.0.ffn_down.weight", (8, 96), "IQ4_NL", S.dequant_fixture(NL, 8, 96).tobytes()),
               ("blk.0.ffn_up.weight", (8, 256), "IQ4_NL", S.dequant_fixture(NL, 8, 256).tobytes())]
    path = tmp_path / "m.gguf"
    path.write_bytes(W.serialise([("general.architecture", "str", "llama")], tensors))
    keep = gguf_loader.packed_linear_tensors(Model(), str(path))
    assert keep == {"model.layers.0.mlp.up_proj": ("blk.0.ffn_up.weight", NL)}
