"""No GPU: the host side of K15 (gq_unpack / gq_dequantize_blocks, gguf_loader, the splitter's HF side) -- ABI surface and
argument checks, the rotary row un-permute, the name maps, and the splitter's file plumbing with the decode injected."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")


def test_cabi_declares_exports_and_checks_the_decode_entry_points():
    from gptq_gguf_toolkit_amd import GQError, _cabi, ops
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf.h")).read()
    raw = ctypes.CDLL(_cabi.SO_PATH)
    for sym in ("gq_unpack", "gq_dequantize_blocks"):
        assert re.search(rf"\bint {sym}\s*\(", hdr) and sym in _cabi.EXPORTS and hasattr(raw, sym)
    lib = _cabi.lib()
    n = None
    assert lib.gq_unpack(12, n, 16, 300, n, n, n, n, n, n) == -2 and b"256" in lib.gq_last_error()
    assert lib.gq_dequantize_blocks(12, n, 16, 300, n, n, _cabi.F16, n) == -2 and b"256" in lib.gq_last_error()
    assert lib.gq_unpack(12, n, 0, 256, n, n, n, n, n, n) == -2
    assert lib.gq_unpack(3, n, 16, 256, n, n, n, n, n, n) == -1
    assert lib.gq_dequantize_blocks(3, n, 16, 256, n, n, _cabi.F16, n) == -1
    assert lib.gq_dequantize_blocks(12, n, 16, 256, n, n, 7, n) == -1 and b"out_dtype" in lib.gq_last_error()
    # two faults: the type's refusal comes before the out_dtype's
    assert lib.gq_dequantize_blocks(9, n, 16, 256, n, n, 7, n) == -1
    assert lib.gq_last_error() == b"gq_dequantize_blocks: unknown q_type 9"
    null = lib.gq_unpack(12, n, 16, 256, n, n, n, n, n, n)
    assert null == lib.gq_dequantize_blocks(12, n, 16, 256, n, n, _cabi.F32, n) == lib.gq_pack(12, n, n, n, n, n, 16, 256, n, n)
    assert null < 0 and b"null" in lib.gq_last_error()
    blocks = torch.zeros(4, 144, dtype=torch.uint8)
    with pytest.raises(GQError):
        ops.unpack(12, blocks)
    with pytest.raises(GQError):
        ops.dequantize_blocks(12, blocks, torch.float16)


@pytest.mark.parametrize("heads", [(32, 32), (32, 8), (4, 2)])
def test_unpermute_inverts_the_converters_permute(heads):
    from gptq_gguf_toolkit_amd.gguf_loader import unpermute, unpermute_rows
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import permute
    h, kv = heads
    for n_kv, R in ((h, h * 8), (kv, kv * 8)):  # a q_proj (h heads) and a k_proj (kv heads) of head_dim 8
        x = torch.randn(R, 24, generator=torch.Generator().manual_seed(R))
        assert torch.equal(unpermute(permute(x, h, n_kv), h, n_kv), x)
        assert torch.equal(permute(unpermute(x, h, n_kv), h, n_kv), x)
        rows = unpermute_rows(R, h, n_kv)
        assert rows.dtype == torch.int32 and rows.shape == (R,) and sorted(rows.tolist()) == list(range(R))
        assert torch.equal(x[rows.long()], unpermute(x, h, n_kv))
        five = x[:, :3].contiguous()  # the converter permutes all five tensors: any trailing shape
        assert torch.equal(unpermute(permute(five, h, n_kv), h, n_kv), five)


def test_hf_tensor_name_inverts_map_tensor_name():
    from gptq_gguf_toolkit_amd.gguf_loader import hf_tensor_name
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import map_tensor_name
    names = ["model.embed_tokens.weight", "model.norm.weight", "lm_head.weight"]
    for i in (0, 7, 31):
        names += [f"model.layers.{i}.{r}.weight" for r in
                  ("input_layernorm", "post_attention_layernorm", "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj",
                   "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")]
    for n in names:
        assert hf_tensor_name(map_tensor_name(n)) == n
    assert len({map_tensor_name(n) for n in names}) == len(names)
    for bad in ("rope_freqs.weight", "blk.0.ffn_gate_exps.weight", "blk.x.attn_q.weight"):
        with pytest.raises(ValueError):
            hf_tensor_name(bad)


def _write_gguf(path, with_experts=False):
    from gptq_gguf_toolkit_amd.gguf_writer import GGMLType, GGUFWriter
    rng = np.random.default_rng(1)
    t = {"blk.0.attn_q.weight": (rng.integers(0, 256, (8, 144), dtype=np.uint8), GGMLType.Q4_K),
         "blk.0.ffn_down.weight": (rng.integers(0, 256, (4, 110), dtype=np.uint8), GGMLType.Q3_K),
         "blk.0.ffn_up.weight": (rng.integers(0, 256, (4, 210), dtype=np.uint8), GGMLType.Q6_K)}
    nrm = rng.standard_normal(8).astype(np.float32)
    w = GGUFWriter(str(path), "llama")
    w.add_uint32("llama.block_count", 1)
    w.add_uint32("llama.attention.head_count", 4)
    w.add_uint32("llama.attention.head_count_kv", 2)
    for k, (a, gt) in t.items():
        w.add_tensor(k, a, raw_dtype=gt)
    w.add_tensor("output_norm.weight", nrm)
    if with_experts:
        w.add_tensor("blk.0.ffn_gate_exps.weight", rng.standard_normal((2, 4, 8)).astype(np.float32))
    w.write()
    return t, nrm


def test_splitter_cli_default_is_unchanged_and_new_flags_parse(tmp_path, monkeypatch):
    from gptq_gguf_toolkit_amd import gguf_splitter as S
    t, nrm = _write_gguf(tmp_path / "m.gguf")
    S.main([str(tmp_path / "m.gguf"), str(tmp_path / "a")])
    S.main([str(tmp_path / "m.gguf"), str(tmp_path / "b"), "--gguf-layers", "--bitwidth", "4"])
    files = lambda d: sorted(str(p.relative_to(d)) for p in d.rglob("*") if p.is_file())  # noqa: E731
    want = sorted(["manifest.json", "gguf_layer_database.json", "blk.0.attn_q.weight/4.pth", "blk.0.attn_q.weight/4-metadata.json",
                   "blk.0.ffn_down.weight/3.pth", "blk.0.ffn_down.weight/3-metadata.json", "blk.0.ffn_up.weight/6.pth",
                   "blk.0.ffn_up.weight/6-metadata.json", "output_norm.weight/32.pth", "output_norm.weight/32-metadata.json"])
    assert files(tmp_path / "a") == files(tmp_path / "b") == want  # no HF-side file without --hf-layers
    assert (tmp_path / "a" / "blk.0.attn_q.weight" / "4.pth").read_bytes() == t["blk.0.attn_q.weight"][0].tobytes()
    assert (tmp_path / "a" / "output_norm.weight" / "32.pth").read_bytes() == nrm.tobytes()
    # --hf-layers / --both reach split_hf_model with the reference's arguments; the GGUF side runs only when asked
    calls = []
    monkeypatch.setattr(S.GGUFSplitter, "split_hf_model",
                        lambda self, dtype, ob, device: calls.append((dtype, ob, device)) or {"mapping_stats": {"total_layers": 0, "mapped_layers": 0}})
    S.main([str(tmp_path / "m.gguf"), str(tmp_path / "c"), "--hf-layers"])
    assert calls == [("float16", None, "cuda:0")] and not (tmp_path / "c" / "gguf_layer_database.json").exists()
    S.main([str(tmp_path / "m.gguf"), str(tmp_path / "d"), "--both", "--dtype", "float32", "--bitwidth", "0", "--device", "cuda:1"])
    assert calls[1] == ("float32", 0, "cuda:1") and (tmp_path / "d" / "gguf_layer_database.json").exists()
    assert [S.hf_overwrite_from_cli(b) for b in (16, "16", "4.5", "Q4_K", "0", "-1")] == [None, None, None, None, 0, 0]
    with pytest.raises(SystemExit):
        S.main([str(tmp_path / "m.gguf"), str(tmp_path / "e"), "--dtype", "bfloat16"])


def test_split_hf_model_tree_and_bitwidth_rule(tmp_path):
    """The reference's output tree (mapper/gguf_splitter.py:487-625) and its overwrite / skip rule (:530-551), the decoded
    tensors injected: file-name stem, metadata and manifest keys, mapping stats, the layer-mapping file."""
    from gptq_gguf_toolkit_amd.gguf_splitter import GGUFSplitter
    _write_gguf(tmp_path / "m.gguf")
    g = torch.Generator().manual_seed(0)
    tensors = [("model.embed_tokens.weight", torch.randn(16, 8, generator=g)),
               ("model.layers.0.self_attn.q_proj.weight", torch.randn(8, 256, generator=g)),
               ("model.layers.0.input_layernorm.weight", torch.randn(8, generator=g)),
               ("model.layers.0.mlp.down_proj.weight", torch.randn(4, 256, generator=g)),
               ("model.layers.0.mlp.up_proj.weight", torch.randn(4, 256, generator=g))]
    sp = GGUFSplitter(str(tmp_path / "m.gguf"), str(tmp_path / "hf"))
    man = sp.split_hf_model("float16", None, tensors=tensors)
    assert man["mapping_stats"] == {"total_layers": 3, "mapped_layers": 3, "unmapped_layers": 0}
    assert set(man["model_info"]) == {"original_file", "dtype", "bitwidth", "use_exact_bitwidth", "split_timestamp"}
    assert man == json.loads((tmp_path / "hf" / "manifest.json").read_text())
    assert json.loads((tmp_path / "hf" / "hf_to_gguf_mapping.json").read_text()) == {
        "model.layers.0.self_attn.q_proj.weight": "blk.0.attn_q.weight", "model.layers.0.mlp.down_proj.weight": "blk.0.ffn_down.weight",
        "model.layers.0.mlp.up_proj.weight": "blk.0.ffn_up.weight"}
    assert sorted(p.name for p in (tmp_path / "hf").iterdir() if p.is_dir()) == [
        "model.layers.0.mlp.down_proj", "model.layers.0.mlp.up_proj", "model.layers.0.self_attn.q_proj"]
    d = tmp_path / "hf" / "model.layers.0.self_attn.q_proj"
    got = torch.load(d / "4-Q4_K.pth", weights_only=True)
    assert got.dtype == torch.float16 and torch.equal(got, tensors[1][1].half())
    meta = json.loads((d / "4-Q4_K-metadata.json").read_text())
    assert set(meta) == {"tensor_info", "gguf_info"} and meta["gguf_info"] == sp.gguf_layer_database["blk.0.attn_q.weight"]
    assert meta["tensor_info"] == {"name": "model.layers.0.self_attn.q_proj.weight", "gguf_mapped_name": "blk.0.attn_q.weight",
                                   "bitwidth": 4, "dtype": "torch.float16", "shape": [8, 256], "n_elements": 2048, "n_bytes": 4096,
                                   "data_filename": "4-Q4_K.pth", "requires_grad": True}
    rec = man["layers"]["model.layers.0.mlp.down_proj.weight"]
    assert rec == {"original_name": "model.layers.0.mlp.down_proj.weight", "gguf_mapped_name": "blk.0.ffn_down.weight",
                   "layer_directory": "model.layers.0.mlp.down_proj", "dims": [4, 256], "bitwidth": 3, "filename": "3-Q3_K.pth",
                   "metadata_filename": "3-Q3_K-metadata.json", "dtype": "torch.float16", "size_bytes": 2048, "shape": [4, 256],
                   "n_elements": 1024}
    # a type name keeps the layers of that bit-width class and skips the others; a number names the file without a type
    sp2 = GGUFSplitter(str(tmp_path / "m.gguf"), str(tmp_path / "hf2"))
    man2 = sp2.split_hf_model("float32", "Q4_K", tensors=tensors)
    assert list(man2["layers"]) == ["model.layers.0.self_attn.q_proj.weight"] and man2["mapping_stats"]["total_layers"] == 3
    assert torch.load(tmp_path / "hf2" / "model.layers.0.self_attn.q_proj" / "4-Q4_K.pth", weights_only=True).dtype == torch.float32
    man3 = GGUFSplitter(str(tmp_path / "m.gguf"), str(tmp_path / "hf3")).split_hf_model("float16", 6, tensors=tensors)
    assert [r["filename"] for r in man3["layers"].values()] == ["6.pth"] and man3["layers"]["model.layers.0.mlp.up_proj.weight"]["bitwidth"] == 6.0
    man4 = GGUFSplitter(str(tmp_path / "m.gguf"), str(tmp_path / "hf4")).split_hf_model("float16", 0, tensors=tensors)
    assert [r["filename"] for r in man4["layers"].values()] == ["0.pth"] * 3  # <= 0: every layer, whatever its GGUF class
    # exact widths; a layer the file does not hold needs an overwrite
    spx = GGUFSplitter(str(tmp_path / "m.gguf"), str(tmp_path / "hf5"), use_exact_bitwidth=True)
    assert spx.split_hf_model("float16", None, tensors=tensors[:2])["layers"]["model.layers.0.self_attn.q_proj.weight"]["filename"] == "4.5-Q4_K.pth"
    extra = [("model.layers.1.self_attn.v_proj.weight", torch.zeros(4, 256))]
    with pytest.raises(ValueError, match="v_proj"):
        GGUFSplitter(str(tmp_path / "m.gguf"), str(tmp_path / "hf6")).split_hf_model("float16", None, tensors=extra)
    man7 = GGUFSplitter(str(tmp_path / "m.gguf"), str(tmp_path / "hf7")).split_hf_model("float16", 5, tensors=extra)
    assert man7["mapping_stats"] == {"total_layers": 1, "mapped_layers": 0, "unmapped_layers": 1}


def test_loader_maps_the_file_and_refuses_what_it_cannot_decode(tmp_path):
    from gptq_gguf_toolkit_amd import gguf_loader
    from gptq_gguf_toolkit_amd.gguf_writer import parse_gguf
    t, nrm = _write_gguf(tmp_path / "m.gguf")
    kv, tensors, buf = parse_gguf(str(tmp_path / "m.gguf"), mmap=True)
    kv2, tensors2, raw = parse_gguf(str(tmp_path / "m.gguf"))
    assert isinstance(buf, np.memmap) and kv == kv2 and tensors == tensors2 and bytes(buf) == raw
    # the K-quant tensors come first: decoding them needs the GPU and is refused on the CPU, loudly
    from gptq_gguf_toolkit_amd import GQError
    with pytest.raises(GQError):
        next(gguf_loader.iter_gguf_tensors(str(tmp_path / "m.gguf"), "cpu"))
    _write_gguf(tmp_path / "moe.gguf", with_experts=True)
    import gptq_gguf_toolkit_amd.ops as ops
    orig = ops.dequantize_blocks
    ops.dequantize_blocks = lambda gt, blocks, dt, rows: torch.zeros(blocks.shape[0], 256, dtype=dt)  # host stand-in
    try:
        it = gguf_loader.iter_gguf_tensors(str(tmp_path / "moe.gguf"), "cpu", torch.float16)
        got = [next(it) for _ in range(4)]
        assert [n for n, _ in got] == ["model.layers.0.self_attn.q_proj.weight", "model.layers.0.mlp.down_proj.weight",
                                       "model.layers.0.mlp.up_proj.weight", "model.norm.weight"]
        assert got[3][1].dtype == torch.float16 and torch.equal(got[3][1], torch.from_numpy(nrm).half())
        with pytest.raises(NotImplementedError, match="ffn_gate_exps"):
            next(it)
    finally:
        ops.dequantize_blocks = orig
    # a ggml type outside the supported set names the tensor and the type
    data = bytearray(open(tmp_path / "m.gguf", "rb").read())
    pos = data.index(b"blk.0.ffn_down.weight") + len(b"blk.0.ffn_down.weight") + 4 + 2 * 8  # n_dims, two dims -> type
    assert int.from_bytes(data[pos:pos + 4], "little") == 11
    data[pos:pos + 4] = (2).to_bytes(4, "little")  # Q4_0
    (tmp_path / "q40.gguf").write_bytes(bytes(data))
    with pytest.raises(ValueError, match=r"blk\.0\.ffn_down\.weight.*type 2"):
        list(gguf_loader.iter_gguf_tensors(str(tmp_path / "q40.gguf"), "cpu"))
