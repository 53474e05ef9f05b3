"""Layer error estimator, the level loader (no GPU): a `--gguf-layers` database made by the package's own splitter from a
GGUF with NON-SQUARE tensors -- a Q4_K attn_k (rotary row permutation), a Q4_K ffn_down, an F16 attn_q -- is read back by
level_db.load_level / layer_dir and must equal what gguf_loader makes of the same file, with ops.dequantize_blocks
replaced in both by one stand-in that keeps every byte and the row gather visible.  Also the torch-saved (--hf-layers) side."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")

R_K, R_D, R_Q, C = 8, 6, 16, 512  # attn_k [8, 512], ffn_down [6, 512], attn_q [16, 512]; 4 heads, 2 kv heads
TS = 144                           # bytes per 256 values of Q4_K


def _fake_dequantize_blocks(q_type, blocks, out_dtype=torch.float32, row_src=None):
    """[R, C/256*type_size] bytes -> [R, C]: value (r, c) is byte (row_src[r], c % row bytes) -- shape, byte order and the
    row gather of the real op, none of its arithmetic."""
    assert q_type == 12 and blocks.dtype == torch.uint8 and blocks.dim() == 2 and blocks.shape[1] % TS == 0
    cols = blocks.shape[1] // TS * 256
    src = blocks if row_src is None else blocks[row_src.long()]
    return src.repeat(1, cols // src.shape[1] + 1)[:, :cols].to(out_dtype)


@pytest.fixture()
def db(tmp_path, monkeypatch):
    from gptq_gguf_toolkit_amd import error_estimator as ee, gguf_loader, level_db as ldb, ops
    from gptq_gguf_toolkit_amd.gguf_splitter import main as split_main
    from gptq_gguf_toolkit_amd.gguf_writer import GGMLType, GGUFWriter
    rng = np.random.default_rng(18)
    k = rng.integers(0, 256, (R_K, C // 256 * TS), dtype=np.uint8)
    d = rng.integers(0, 256, (R_D, C // 256 * TS), dtype=np.uint8)
    q = rng.standard_normal((R_Q, C)).astype(np.float16)
    w = GGUFWriter(str(tmp_path / "m.gguf"), "llama")
    w.add_uint32("llama.block_count", 1)
    w.add_uint32("llama.attention.head_count", 4)
    w.add_uint32("llama.attention.head_count_kv", 2)
    w.add_tensor("blk.0.attn_k.weight", k, raw_dtype=GGMLType.Q4_K)
    w.add_tensor("blk.0.ffn_down.weight", d, raw_dtype=GGMLType.Q4_K)
    w.add_tensor("blk.0.attn_q.weight", q)
    w.write()
    split_main([str(tmp_path / "m.gguf"), str(tmp_path / "db"), "--exact", "--gguf-layers"])
    monkeypatch.setattr(ops, "dequantize_blocks", _fake_dequantize_blocks)  # the ops level_db uses is gguf_loader.ops
    assert gguf_loader.ops is ops
    want = dict(gguf_loader.iter_gguf_tensors(str(tmp_path / "m.gguf"), "cpu", torch.float16, hf_layout=True))
    return ee, ldb, str(tmp_path / "db"), want, (k, d, q)


def test_packed_gguf_levels_decode_as_the_loader_does(db):
    _, ldb, path, want, (k, d, q) = db
    for hf, gg, shape in (("model.layers.0.self_attn.k_proj", "blk.0.attn_k.weight", (R_K, C)),
                          ("model.layers.0.mlp.down_proj", "blk.0.ffn_down.weight", (R_D, C)),
                          ("model.layers.0.self_attn.q_proj", "blk.0.attn_q.weight", (R_Q, C))):
        ldir = ldb.layer_dir(path, hf)  # no directory under the HF name: the GGUF tensor's
        assert os.path.basename(ldir) == gg
        files = ldb.level_files(ldir)
        assert len(files) == 1 and files[0].endswith(".pth")
        got = ldb.load_level(os.path.join(ldir, files[0]), "cpu", path)
        assert tuple(got.shape) == shape and got.dtype == torch.float16
        assert torch.equal(got, want[hf + ".weight"]), hf
    # the rotary un-permute really moved rows of k and q, and left ffn_down alone
    plain_k = _fake_dequantize_blocks(12, torch.from_numpy(k), torch.float16)
    assert not torch.equal(want["model.layers.0.self_attn.k_proj.weight"], plain_k)
    assert torch.equal(want["model.layers.0.mlp.down_proj.weight"], _fake_dequantize_blocks(12, torch.from_numpy(d), torch.float16))
    assert not torch.equal(want["model.layers.0.self_attn.q_proj.weight"], torch.from_numpy(q))
    # without the manifest (db=None) the rows stay as stored
    ldir = ldb.layer_dir(path, "model.layers.0.self_attn.k_proj")
    assert torch.equal(ldb.load_level(os.path.join(ldir, ldb.level_files(ldir)[0]), "cpu"), plain_k)
    with pytest.raises(FileNotFoundError):
        ldb.layer_dir(path, "model.layers.0.mlp.up_proj")


def test_packed_level_reaches_estimate_with_the_layers_shape(db):
    """A non-square packed level goes through LayerErrorEstimator.estimate (shape check included) on fp64 stand-ins."""
    ee, ldb, path, want, _ = db
    import types
    calls = []

    def quad_form(A, H, B=None, ws=None):
        calls.append(None if B is None else tuple(B.shape))
        D = (A.float() - B.float()).double() if B is not None else A.double()
        return ((D @ H.double()) * D).sum()

    fake = types.SimpleNamespace(quad_form=quad_form, dequantize_blocks=_fake_dequantize_blocks,
                                 h_accumulate=lambda H, X, b, a, ws=None: H.copy_(b * H + a * (X.float().T @ X.float())))
    old, ee._ops = ee._ops, fake
    try:
        layer = torch.nn.Linear(C, R_K, bias=False)
        h = ee.LayerErrorEstimator(layer)
        h.update(torch.randn(1, 2 * C, C))
        h.pre_step()
        ldir = ldb.layer_dir(path, "model.layers.0.self_attn.k_proj")
        w_c = ldb.load_level(os.path.join(ldir, ldb.level_files(ldir)[0]), "cpu", path)
        v = h.estimate(w_c)
        assert v.dtype == torch.float64 and float(v) > 0 and calls == [(R_K, C), None]
    finally:
        ee._ops = old


def test_torch_saved_levels_load_as_they_are(tmp_path):
    from gptq_gguf_toolkit_amd import level_db as ldb
    d = tmp_path / "model.layers.0.mlp.up_proj"
    d.mkdir()
    w = torch.randn(6, 256).half()
    torch.save(w, str(d / "4-Q4_K.pth"))
    (d / "4-Q4_K-metadata.json").write_text('{"tensor_info": {"name": "model.layers.0.mlp.up_proj.weight", "shape": [6, 256]}}')
    assert ldb.layer_dir(str(tmp_path), "model.layers.0.mlp.up_proj") == str(d)
    assert torch.equal(ldb.load_level(str(d / "4-Q4_K.pth"), "cpu", str(tmp_path)), w)
