"""The write side of the level database (level_db.LevelDbWriter) against the splitter it replaces, the readers on what it
wrote, its all-or-nothing rule, the HF -> GGUF row order as an index (gguf_loader.rotary_row_dst) and the pure plan of a
gq_pack_bands call (ops.pack_bands_plan).  No GPU."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

OFFSET_KEYS = ("data_offset", "data_offset_original")
TS = {10: 84, 11: 110, 12: 144, 13: 176, 14: 210}
R, C = 8, 512


def _strip(d):
    return {k: v for k, v in d.items() if k not in OFFSET_KEYS}


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """One small .gguf from the package's GGUFWriter -- every K-quant type as random bytes, an F32 vector, an F16 matrix, scalar
    and array key/value entries -- split with --exact, and the same tensors and key/value data fed through the writer."""
    from gptq_gguf_toolkit_amd import level_db
    from gptq_gguf_toolkit_amd.gguf_splitter import GGUFSplitter
    from gptq_gguf_toolkit_amd.gguf_writer import GGUFValueType, GGUFWriter, kv_records
    tmp = tmp_path_factory.mktemp("level_db_write")
    rng = np.random.default_rng(31)
    tensors = [("rope_freqs.weight", rng.standard_normal(32).astype(np.float32), None)]
    for i, t in enumerate(TS):
        tensors.append((f"blk.0.t{i}.weight", rng.integers(0, 256, (R, C // 256 * TS[t]), dtype=np.uint8), t))
    tensors.append(("token_embd.weight", rng.standard_normal((R, C)).astype(np.float16), None))
    w = GGUFWriter(str(tmp / "m.gguf"), "llama")
    w.add_string("general.name", "tiny")
    w.add_uint32("llama.block_count", 1)
    w.add_float32("llama.attention.layer_norm_rms_epsilon", 1e-5)  # no float32: comes back from a file as its nearest one
    w.add_bool("tokenizer.ggml.add_bos_token", True)
    w.add_array("tokenizer.ggml.tokens", ["<s>", "a", "▁b"], GGUFValueType.STRING)
    w.add_array("tokenizer.ggml.scores", [0.0, -1.5, -1e-5], GGUFValueType.FLOAT32)
    w.add_array("tokenizer.ggml.token_type", [3, 1, 1], GGUFValueType.INT32)
    for name, data, raw in tensors:
        w.add_tensor(name, data, raw_dtype=raw)
    w.write()
    split = GGUFSplitter(str(tmp / "m.gguf"), str(tmp / "split"), use_exact_bitwidth=True)
    split.split_gguf_model()
    wr = level_db.LevelDbWriter(str(tmp / "db"))
    for name, data, raw in reversed(tensors):  # another order than the file's: close() orders
        gt = raw if raw is not None else {np.dtype(np.float32): 0, np.dtype(np.float16): 1}[data.dtype]
        shape = (data.shape[0], data.shape[1] // TS[raw] * 256) if raw is not None else data.shape
        wr.add_level(name, shape, gt, data)
    wr.set_metadata(kv_records(w.kv))
    wr.set_order([name for name, _, _ in tensors])
    assert not os.path.exists(tmp / "db") and os.path.isdir(str(tmp / "db") + ".partial")
    assert wr.close() == str(tmp / "db") and not os.path.exists(str(tmp / "db") + ".partial")
    return tmp / "split", tmp / "db", tensors


def test_writer_equals_splitter(pair):
    split, db, tensors = pair
    files = sorted(os.path.relpath(os.path.join(d, f), split) for d, _, fs in os.walk(split) for f in fs)
    assert files == sorted(os.path.relpath(os.path.join(d, f), db) for d, _, fs in os.walk(db) for f in fs)
    assert sum(f.endswith(".pth") for f in files) == len(tensors) == 7
    for f in files:
        a, b = open(split / f, "rb").read(), open(db / f, "rb").read()
        if f.endswith(".pth"):
            assert a == b, f
        elif f.endswith("-metadata.json"):
            ja, jb = json.loads(a)["tensor_info"], json.loads(b)["tensor_info"]
            assert set(ja) - set(jb) == {"data_offset_original"} and list(_strip(ja).items()) == list(jb.items()), f
    ma, mb = json.load(open(split / "manifest.json")), json.load(open(db / "manifest.json"))
    assert ma["metadata"] == mb["metadata"] and list(ma["metadata"]) == list(mb["metadata"])
    assert mb["metadata"]["tokenizer.ggml.scores"]["types"] == [9, 6] and mb["metadata"]["llama.block_count"] == {"types": [4], "value": 1}
    assert mb["metadata"]["llama.attention.layer_norm_rms_epsilon"]["value"] == float(np.float32(1e-5))
    assert "original_file" not in mb["model_info"] and mb["model_info"]["use_exact_bitwidth"] is True
    assert list(ma["layers"]) == list(mb["layers"]) == [name for name, _, _ in tensors]
    for name in ma["layers"]:
        la, lb = ma["layers"][name], mb["layers"][name]
        assert {k: v for k, v in la.items() if k != "bitwidths"} == {k: v for k, v in lb.items() if k != "bitwidths"}
        assert list(la["bitwidths"]) == list(lb["bitwidths"])
        for bw in la["bitwidths"]:
            assert list(_strip(la["bitwidths"][bw]).items()) == list(lb["bitwidths"][bw].items()), (name, bw)
    da, dbj = json.load(open(split / "gguf_layer_database.json")), json.load(open(db / "gguf_layer_database.json"))
    assert list(da) == list(dbj)
    for name in da:
        assert list(_strip(da[name]).items()) == list(dbj[name].items()), name


def test_all_levels_of_a_tensor_are_listed_and_the_last_is_its_database_record(tmp_path):
    from gptq_gguf_toolkit_amd import level_db
    rng = np.random.default_rng(32)
    with level_db.LevelDbWriter(str(tmp_path / "db")) as wr:
        for t in (10, 12, 14):
            wr.add_level("blk.0.ffn_up.weight", (R, C), t, rng.integers(0, 256, (R, C // 256 * TS[t]), dtype=np.uint8))
    m = json.load(open(tmp_path / "db" / "manifest.json"))
    assert list(m["layers"]["blk.0.ffn_up.weight"]["bitwidths"]) == ["2.5625", "4.5", "6.5625"]
    assert [v["filename"] for v in m["layers"]["blk.0.ffn_up.weight"]["bitwidths"].values()] == ["2.5625-Q2_K.pth", "4.5-Q4_K.pth",
                                                                                              "6.5625-Q6_K.pth"]
    rec = json.load(open(tmp_path / "db" / "gguf_layer_database.json"))["blk.0.ffn_up.weight"]
    assert rec["quantization"] == "Q6_K" and rec["n_bytes"] == R * C // 256 * 210 and "data_offset" not in rec
    with pytest.raises(FileExistsError):
        level_db.LevelDbWriter(str(tmp_path / "db"))


def test_readers_and_the_stitcher_accept_the_written_database(pair, tmp_path):
    from gptq_gguf_toolkit_amd import level_db
    from gptq_gguf_toolkit_amd.gguf_stitcher import GGUFStitcher
    _, db, tensors = pair
    avail = level_db.scan_available_bitwidths(str(db))
    assert set(avail) == {name for name, _, _ in tensors}
    for name, data, raw in tensors:
        (bw, fname), = avail[name]
        rec = level_db.read_sidecar(str(db / name / fname))
        assert level_db.check_level_size(rec) == data.nbytes and rec.name == name
        assert rec.ggml_type == (raw if raw is not None else {4: 0, 2: 1}[data.itemsize])
        assert np.array_equal(level_db.read_level_raw(rec), data.reshape(-1).view(np.uint8))
    st = GGUFStitcher(str(db), None, str(tmp_path / "out.gguf"), quiet=True)
    assert st.original_metadata is None  # no original_file: the manifest's key/value data is the source
    planned = st.plan()
    assert [p.name for p in planned] == [name for name, _, _ in tensors]
    assert [p.nbytes for p in planned] == [data.nbytes for _, data, _ in tensors]


def test_nothing_half_written(tmp_path):
    from gptq_gguf_toolkit_amd import level_db
    db = tmp_path / "db"
    with pytest.raises(RuntimeError, match="boom"):
        with level_db.LevelDbWriter(str(db)) as wr:
            wr.add_level("blk.0.ffn_up.weight", (R, C), 12, np.zeros((R, C // 256 * 144), np.uint8))
            raise RuntimeError("boom")
    assert not db.exists() and not os.path.exists(str(db) + ".partial")
    # a booked file that never arrived, or arrived short, fails close() -- and leaves nothing either
    for data in (None, np.zeros(7, np.uint8)):
        wr = level_db.LevelDbWriter(str(db))
        path = wr.register("blk.0.ffn_up.weight", (R, C), 12)
        if data is not None:
            data.tofile(path)
        with pytest.raises((FileNotFoundError, ValueError)):
            wr.close()
        assert not db.exists() and not os.path.exists(str(db) + ".partial")


@pytest.mark.parametrize("n_head,n_kv", [(4, 4), (4, 2), (8, 1)])
def test_rotary_row_dst_is_permute_as_an_index(n_head, n_kv):
    from gptq_gguf_toolkit_amd.gguf_loader import rotary_row_dst, rotary_row_src
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import permute
    for name, heads in (("blk.3.attn_q.weight", n_head), ("blk.3.attn_k.weight", n_kv)):
        rows = heads * 16
        dst = rotary_row_dst(name, rows, n_head, n_kv, "cpu")
        ident = torch.arange(rows, dtype=torch.int32)
        assert dst.dtype == torch.int32 and torch.equal(dst, permute(ident, n_head, heads))
        x = torch.randn(rows, 3)
        assert torch.equal(x[dst.long()], permute(x, n_head, heads))
        src = rotary_row_src(name, rows, "llama", n_head, n_kv, "cpu")
        assert torch.equal(dst[src.long()], ident) and torch.equal(src[dst.long()], ident)
        assert rotary_row_dst(name, rows, n_head, n_kv, "cpu") is dst  # one tensor per (q or k, R)
    assert rotary_row_dst("blk.3.attn_v.weight", 64, n_head, n_kv, "cpu") is None


def test_pack_bands_plan():
    from gptq_gguf_toolkit_amd import ops
    bands = [(64, 10), (128, 11), (256, 12), (320, 13), (448, 14)]
    plan, total = ops.pack_bands_plan(bands, 512)
    off = 0
    for (r0, r1, t, row_bytes, nbytes, o), (end, bt), start in zip(plan, bands, (0, 64, 128, 256, 320)):
        assert (r0, r1, t) == (start, end, bt) and row_bytes == 2 * TS[bt] and nbytes == (r1 - r0) * row_bytes
        assert o == off and o % 16 == 0
        off += nbytes
    assert total == off == 64 * 168 + 64 * 220 + 128 * 288 + 64 * 352 + 128 * 420
    for bad, c in (([(128, 12), (64, 10)], 512), ([(96, 12)], 512), ([(64, 12)], 384), ([(64, 12)], 0),
                   ([(64 * (k + 1), 12) for k in range(ops.BANDS_MAX + 1)], 256), ([(64, 9)], 256), ([], 256)):
        with pytest.raises(ValueError):
            ops.pack_bands_plan(bad, c)
    assert len(ops.pack_bands_plan([(64 * (k + 1), 12) for k in range(ops.BANDS_MAX)], 256)[0]) == 64


def test_header_and_binding_name_the_same_symbol():
    import re
    from conftest import ROOT
    from gptq_gguf_toolkit_amd import _cabi
    text = open(os.path.join(ROOT, "include", "gptq_gguf_levelpack.h")).read()
    declared = set(re.findall(r"^int (gq_\w+)\(", text, re.M))
    assert declared == set(_cabi.EXPORTS_LEVELPACK) == {"gq_pack_bands"}
    assert int(re.search(r"#define GQ_PACK_BANDS_ALIGN (\d+)", text).group(1)) == _cabi.PACK_BANDS_ALIGN == 16
    assert '#include "gptq_gguf_levels.h"' in text and "GQ_ABI_VERSION does not change" in text
