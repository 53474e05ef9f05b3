"""level_db, the one reader of the per-layer level database (no GPU): the two file-name rules and the one formatter pinned
on the values the functions they replace gave, the sidecar record of every kind of level in a database made by the
package's own splitter, the size check, and the head-count rule of the manifest.  A stored level through LevelStore against
load_level needs ops.level_switch, which has no stand-in here: tests/test_gpu_search.py keeps that comparison."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

R_K, R_Q, C, TS = 8, 16, 512, 144  # attn_k [8, 512] Q4_K (144 bytes per 256 values), attn_q [16, 512] F16; 4 heads, 2 kv heads

NAMES = [  # file name, level_key, parse_level_name (ValueError: the rule refuses the name)
    ("4.pth", 4.0, (4.0, None)),
    ("4-Q4_K.pth", 4.0, (4.0, "Q4_K")),
    ("4.5-Q4_K.pth", 4.5, (4.5, "Q4_K")),
    ("2.5625-Q2_K.pth", 2.5625, (2.5625, "Q2_K")),
    ("10.pth", 10.0, (10.0, None)),
    ("0.pth", 0.0, (0.0, None)),
    ("32-F32.pth", 32.0, (32.0, "F32")),
    ("best.pth", ValueError, None),
    ("4-Q4_K.extra.pth", 4.0, None),
    ("4-Q4_K-metadata.json", 4.0, None),
    ("4..5.pth", 4.0, ValueError),
    (".5.pth", ValueError, (0.5, None)),
]


@pytest.mark.parametrize("rule, column", [("level_key", 1), ("parse_level_name", 2)])
def test_the_two_name_rules_keep_their_values(rule, column):
    from gptq_gguf_toolkit_amd import level_db
    for row in NAMES:
        name, want = row[0], row[column]
        if want is ValueError:
            with pytest.raises(ValueError):
                getattr(level_db, rule)(name)
        else:
            got = getattr(level_db, rule)(name)
            assert got == want and type(got) is type(want), (rule, name, got)


def test_level_stem_is_the_one_formatter():
    from gptq_gguf_toolkit_amd.level_db import level_stem
    assert [level_stem(b) for b in (4, 4.0, 0, 16)] == ["4", "4", "0", "16"]
    assert level_stem(4.5, "Q4_K") == "4.5-Q4_K" and level_stem(4, "Q4_K") == "4-Q4_K"
    assert level_stem(2.5625, "Q2_K") == "2.5625-Q2_K" and level_stem(4.5) == "4.5"


def test_match_level_and_find_level_file(tmp_path):
    from gptq_gguf_toolkit_amd import level_db
    pairs = [(2.5625, "a"), (4.5, "b"), (4.5, "c")]
    assert level_db.match_level(pairs, 4.5 + 5e-7) == "b" and level_db.match_level(pairs, 4.5 + 2e-6) is None
    assert level_db.filename_of({"x": pairs}, "x", 2.5625) == "a"
    for f in ("4-Q4_K.pth", "4.5-Q4_K.pth", "4.5-Q5_K.pth", "3.pth"):
        (tmp_path / f).write_bytes(b"")
    find = lambda level: os.path.basename(level_db.find_level_file(str(tmp_path), level))  # noqa: E731
    assert [find(lv) for lv in (3, "3.0", " 4 ", "4-Q4_K", "4.5-Q5_K")] == ["3.pth", "3.pth", "4-Q4_K.pth", "4-Q4_K.pth",
                                                                          "4.5-Q5_K.pth"]
    with pytest.raises(FileNotFoundError, match="4.5-Q4_K"):  # the number alone names two files
        find(4.5)
    assert level_db.level_files(str(tmp_path)) == ["3.pth", "4-Q4_K.pth", "4.5-Q4_K.pth", "4.5-Q5_K.pth"]


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    """A --gguf-layers --exact database of two layers from the package's own splitter, plus two torch-saved levels written
    by hand: one without a sidecar, one with the HF side's sidecar (no np_dtype)."""
    from gptq_gguf_toolkit_amd.gguf_splitter import main as split_main
    from gptq_gguf_toolkit_amd.gguf_writer import GGMLType, GGUFWriter
    tmp = tmp_path_factory.mktemp("level_db")
    rng = np.random.default_rng(20)
    k = rng.integers(0, 256, (R_K, C // 256 * TS), dtype=np.uint8)
    q = rng.standard_normal((R_Q, C)).astype(np.float16)
    w = GGUFWriter(str(tmp / "m.gguf"), "llama")
    w.add_uint32("llama.block_count", 1)
    w.add_uint32("llama.attention.head_count", 4)
    w.add_uint32("llama.attention.head_count_kv", 2)
    w.add_tensor("blk.0.attn_k.weight", k, raw_dtype=GGMLType.Q4_K)
    w.add_tensor("blk.0.attn_q.weight", q)
    w.write()
    split_main([str(tmp / "m.gguf"), str(tmp / "db"), "--exact", "--gguf-layers"])
    hf = tmp / "db" / "model.layers.0.mlp.up_proj"
    hf.mkdir()
    dense = torch.randn(6, 256).half()
    torch.save(dense, str(hf / "4-Q4_K.pth"))
    torch.save(dense, str(hf / "6-Q6_K.pth"))
    (hf / "6-Q6_K-metadata.json").write_text(json.dumps({"tensor_info": {
        "name": "model.layers.0.mlp.up_proj.weight", "gguf_mapped_name": "blk.0.ffn_up.weight", "bitwidth": 6,
        "dtype": "torch.float16", "shape": [6, 256], "n_elements": 1536, "n_bytes": 3072, "data_filename": "6-Q6_K.pth"}}))
    return tmp / "db", k, q, dense


def test_one_sidecar_reader_describes_every_kind_of_level(db):
    from gptq_gguf_toolkit_amd import level_db
    path, k, q, dense = db
    rec = level_db.read_sidecar(str(path / "blk.0.attn_k.weight" / "4.5-Q4_K.pth"))
    assert (rec.ggml_type, rec.np_dtype, rec.np_shape, rec.shape, rec.nbytes) == (12, "uint8", [R_K, C // 256 * TS], (R_K, C), k.nbytes)
    assert (rec.name, rec.quantization) == ("blk.0.attn_k.weight", "Q4_K")
    assert level_db.check_level_size(rec) == k.nbytes and np.array_equal(level_db.read_level_raw(rec).reshape(k.shape), k)
    rec = level_db.read_sidecar(str(path / "blk.0.attn_q.weight" / "16-F16.pth"))
    assert (rec.ggml_type, rec.np_dtype, rec.np_shape, rec.shape, rec.nbytes) == (1, "float16", [R_Q, C], (R_Q, C), q.nbytes)
    assert level_db.check_level_size(rec) == q.nbytes and np.array_equal(level_db.read_level_raw(rec).view(np.float16).reshape(q.shape), q)
    # torch-saved levels: no sidecar, and the HF side's sidecar, are the same record apart from what names the tensor
    hf = path / "model.layers.0.mlp.up_proj"
    bare, hf_side = level_db.read_sidecar(str(hf / "4-Q4_K.pth")), level_db.read_sidecar(str(hf / "6-Q6_K.pth"))
    for rec in (bare, hf_side):
        assert (rec.ggml_type, rec.np_dtype, rec.np_shape, rec.shape, rec.nbytes) == (None, None, None, None, None)
        assert torch.equal(level_db.load_level(rec.path, "cpu", str(path)), dense)
    assert bare.name == "" and hf_side.name == "model.layers.0.mlp.up_proj.weight"
    # a plain level needs no kernel: the stored rows, and with the manifest the rows in HF order
    stored = level_db.load_level(str(path / "blk.0.attn_q.weight" / "16-F16.pth"), "cpu")
    assert torch.equal(stored, torch.from_numpy(q))
    rows = level_db.rotary_rows(str(path), "blk.0.attn_q.weight", R_Q, "cpu")
    assert torch.equal(level_db.load_level(str(path / "blk.0.attn_q.weight" / "16-F16.pth"), "cpu", str(path)), stored[rows.long()])


def test_size_check_refuses_a_file_one_byte_short(db, tmp_path):
    from gptq_gguf_toolkit_amd import level_db
    src = db[0] / "blk.0.attn_k.weight"
    for f in ("4.5-Q4_K.pth", "4.5-Q4_K-metadata.json"):
        (tmp_path / f).write_bytes((src / f).read_bytes())
    rec = level_db.read_sidecar(str(tmp_path / "4.5-Q4_K.pth"))
    assert level_db.check_level_size(rec) == R_K * C // 256 * TS
    (tmp_path / "4.5-Q4_K.pth").write_bytes((src / "4.5-Q4_K.pth").read_bytes()[:-1])

    class Refused(Exception):
        pass

    for error in (ValueError, Refused):  # the caller chooses the exception type (the stitcher's is its own)
        with pytest.raises(error, match=f"{R_K * C // 256 * TS - 1} bytes on disk"):
            level_db.check_level_size(rec, error)


def test_head_count_list_follows_the_loaders_rule(db, tmp_path):
    from gptq_gguf_toolkit_amd import level_db
    from gptq_gguf_toolkit_amd.gguf_loader import unpermute_rows
    manifest = level_db.read_manifest(str(db[0]))
    assert manifest["metadata"]["llama.attention.head_count"]["value"] == 4
    assert level_db.read_manifest(str(tmp_path)) is None
    assert list(level_db.read_manifest(str(db[0]), "gguf_layer_database.json")) == ["blk.0.attn_k.weight", "blk.0.attn_q.weight"]

    def rows(name, R, head_count=None, head_count_kv=None):
        md = json.loads(json.dumps(manifest))
        if head_count is not None:
            md["metadata"]["llama.attention.head_count"]["value"] = head_count
        if head_count_kv is not None:
            md["metadata"]["llama.attention.head_count_kv"]["value"] = head_count_kv
        (tmp_path / "manifest.json").write_text(json.dumps(md))
        return level_db.rotary_rows(str(tmp_path), name, R, "cpu")

    scalar_q, scalar_k = rows("blk.0.attn_q.weight", R_Q), rows("blk.0.attn_k.weight", R_K)
    assert torch.equal(scalar_q, unpermute_rows(R_Q, 4, 4)) and torch.equal(scalar_k, unpermute_rows(R_K, 4, 2))
    assert not torch.equal(scalar_q, torch.arange(R_Q, dtype=torch.int32)) and scalar_k.dtype == torch.int32
    assert torch.equal(rows("blk.0.attn_q.weight", R_Q, [4, 4, 4]), scalar_q)
    assert torch.equal(rows("blk.0.attn_k.weight", R_K, [4, 4], [2, 2]), scalar_k)
    with pytest.raises(NotImplementedError, match="head_count differs"):
        rows("blk.0.attn_q.weight", R_Q, [4, 8])
    with pytest.raises(NotImplementedError, match="head_count_kv differs"):
        rows("blk.0.attn_k.weight", R_K, 4, [2, 1])
    assert rows("blk.0.ffn_down.weight", R_K, [4, 8]) is None  # not a rotary tensor: the manifest is not even opened
