"""-m gpu: the file the stitcher writes is the model the search scored.  The tiny Llama (hidden 256, 2 layers, 4 heads / 2 KV
heads, vocab 512, fp16: one full 256-column super-block per row, a q / k rotary row permutation that differs between q and
k), three RTN levels per Linear written as three GGUF files with the converter's own name mapping and permutation, split
into one database, a fixed mixed assignment written by the search's configuration_text, stitched with verify=True.  Every
weight equality is on bits; the anchor is LevelStore.switch, which tests/test_gpu_search.py pins to the reference's load path."""
import copy
import os
import shutil
import sys

import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

LEVELS = ((10, 2.5625, "Q2_K"), (12, 4.5, "Q4_K"), (14, 6.5625, "Q6_K"))
LINEARS = r"((q|k|v|o|gate|up|down)_proj)$"


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def write_level(model, names, ggml_type, path):
    """One GGUF of the model with its 14 Linears RTN-quantized to `ggml_type`: pack_gptq_into_gguf's tensor names and q / k
    row permutation, norms F32, the rest F16 (what convert() writes with --outtype f16)."""
    from gptq_gguf_toolkit_amd import ops
    from gptq_gguf_toolkit_amd.gguf_writer import GGUFWriter
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import map_tensor_name, permute
    cfg = model.config
    w = GGUFWriter(str(path), "llama")
    w.add_string("general.name", "tiny-llama")
    w.add_uint32("llama.block_count", cfg.num_hidden_layers)
    w.add_uint32("llama.context_length", cfg.max_position_embeddings)
    w.add_uint32("llama.embedding_length", cfg.hidden_size)
    w.add_uint32("llama.feed_forward_length", cfg.intermediate_size)
    w.add_uint32("llama.attention.head_count", cfg.num_attention_heads)
    w.add_uint32("llama.attention.head_count_kv", cfg.num_key_value_heads)
    w.add_float32("llama.attention.layer_norm_rms_epsilon", cfg.rms_norm_eps)
    w.add_uint32("general.file_type", 1)
    w.add_uint32("general.quantization_version", 2)
    for name, t in model.state_dict().items():
        t = t.detach()
        if name.endswith("q_proj.weight"):
            t = permute(t, cfg.num_attention_heads, cfg.num_attention_heads)
        elif name.endswith("k_proj.weight"):
            t = permute(t, cfg.num_attention_heads, cfg.num_key_value_heads)
        if name[:-len(".weight")] in names:
            packed = ops.pack(ggml_type, *ops.rtn_quantize(t.contiguous(), ggml_type))
            w.add_tensor(map_tensor_name(name), packed.cpu().numpy(), raw_dtype=ggml_type)
        elif t.dim() == 1:
            w.add_tensor(map_tensor_name(name), t.float().cpu().numpy())
        else:
            w.add_tensor(map_tensor_name(name), t.half().cpu().numpy())
    w.write()
    return str(path)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import re
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd import evo_quant_search as S, gguf_splitter
    from gptq_gguf_toolkit_amd.gguf_stitcher import stitch_search_result
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    tmp = tmp_path_factory.mktemp("stitch")
    model = tiny_llama(dtype=torch.float16).cuda()
    names = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and re.search(LINEARS, n)]
    assert len(names) == 14
    files = {tag: write_level(model, names, t, tmp / f"{tag}.gguf") for t, _, tag in LEVELS}
    db, gg = tmp / "db", tmp / "gg"
    for path in files.values():
        gguf_splitter.main([path, str(db), "--both", "--exact", "--dtype", "float16"])  # the search's database, both sides
        gguf_splitter.main([path, str(gg), "--gguf-layers", "--exact"])                 # the GGUF side alone, with its manifest
    # a fixed mixed assignment in place of a search: all three levels, q and k of block 0 on different ones
    widths = [bw for _, bw, _ in LEVELS]
    assignment = {n: widths[(i + i // 7) % 3] for i, n in enumerate(names)}
    assert assignment["model.layers.0.self_attn.q_proj"] == 2.5625 and assignment["model.layers.0.self_attn.k_proj"] == 4.5
    assignment["model.layers.0.self_attn.k_proj"] = 6.5625
    assert set(assignment.values()) == set(widths)
    levels = S.scan_available_bitwidths(str(db), names)
    assert all([f for _, f in levels[n]] == ["2.5625-Q2_K.pth", "4.5-Q4_K.pth", "6.5625-Q6_K.pth"] for n in names)
    cfg = db / S.configuration_name("kl", 4.5)
    cfg.write_text(S.configuration_text([names], [[assignment[n] for n in names]], levels))
    out = stitch_search_result(str(db), str(cfg), str(tmp / "mixed.gguf"), original_model=files["Q4_K"], verify=True)
    return {"model": model, "names": names, "tmp": tmp, "db": db, "gg": gg, "files": files, "assignment": assignment,
            "cfg": cfg, "out": str(out), "calib": tiny_calib()}


def test_stitched_file_is_the_model_the_search_scored(world):
    from gptq_gguf_toolkit_amd import gguf_loader, metrics
    from gptq_gguf_toolkit_amd.gguf_writer import parse_gguf
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import map_tensor_name
    assert os.path.exists(world["out"]) and not os.path.exists(world["out"] + ".partial")
    _, tensors, _ = parse_gguf(world["out"])
    types = {n: gt for n, _, gt, _, _ in tensors}
    by_width = {bw: t for t, bw, _ in LEVELS}
    for n, bw in world["assignment"].items():  # every Linear is stored as the level the configuration names
        assert types[map_tensor_name(n + ".weight")] == by_width[bw], n
    assert [n for n, *_ in tensors] == [n for n, *_ in parse_gguf(world["files"]["Q4_K"])[1]]  # the original's tensor order
    loaded = gguf_loader.load_into_model(copy.deepcopy(world["model"]), world["out"])
    nll = metrics.nll_rows(loaded, world["calib"])
    assert bool(torch.isfinite(nll).all())
    for side in ("gg", "db"):  # the GGUF side (packed bytes, row gather in the switch) and the HF side (dense fp16 files)
        switched = copy.deepcopy(world["model"])
        # the 14 Linears by name: left to itself the store would also take lm_head, whose directory both sides have
        store = LevelStore(switched, str(world[side]), "cuda", layer_names=world["names"])
        assert list(store.layers) == world["names"] and store.switch(world["assignment"]) == 14
        packed = store.find(world["names"][0], 2.5625).kind is not None
        assert packed == (side == "gg")
        for n in world["names"]:
            a, b = loaded.get_submodule(n).weight.data, switched.get_submodule(n).weight.data
            assert torch.equal(bits(a), bits(b)), (side, n)
            assert not torch.equal(bits(a), bits(world["model"].get_submodule(n).weight.data)), n  # and it IS quantized
        for (k, a), (_, b) in zip(loaded.state_dict().items(), switched.state_dict().items()):
            assert torch.equal(bits(a), bits(b)), (side, k)
        assert torch.equal(bits(metrics.nll_rows(switched, world["calib"])), bits(nll)), side


def test_verify_names_the_tensor_that_differs(world, tmp_path, capsys):
    from gptq_gguf_toolkit_amd import config_converter as C, gguf_stitcher
    from gptq_gguf_toolkit_amd.gguf_writer import parse_gguf
    text = C.config_text(C.convert_hf_to_gguf_config(world["cfg"].read_text()))
    (tmp_path / "gguf_config.txt").write_text(text)
    argv = [str(world["db"]), str(tmp_path / "cli.gguf"), "--config", str(tmp_path / "gguf_config.txt"), "--original-model",
            world["files"]["Q4_K"]]
    assert gguf_stitcher.main(argv + ["--verify", "--llama-ftype"]) == 0  # the command-line path, clean
    assert "Verified 21 tensors" in capsys.readouterr().out
    assert open(tmp_path / "cli.gguf", "rb").read() != open(world["out"], "rb").read()  # file_type differs ...
    assert [t[1:] for t in parse_gguf(str(tmp_path / "cli.gguf"))[1]] == [t[1:] for t in parse_gguf(world["out"])[1]]  # ... only

    # one bit of one 4-bit quant of blk.1.attn_v (Q4_K: fp16 d, fp16 dmin, 12 scale bytes, then 128 bytes of quants -- byte 20
    # of the tensor's second block lies among the quants, so no scale changes and nothing non-finite is made)
    victim = "blk.1.attn_v.weight"
    assert world["assignment"]["model.layers.1.self_attn.v_proj"] == 4.5
    flipped = tmp_path / "flipped.gguf"
    shutil.copyfile(world["out"], flipped)
    off = next(o for n, _, gt, o, _ in parse_gguf(str(flipped))[1] if n == victim and gt == 12)
    with open(flipped, "r+b") as f:
        f.seek(off + 144 + 20)
        b = f.read(1)[0]
        f.seek(off + 144 + 20)
        f.write(bytes([b ^ 0x01]))
    st = gguf_stitcher.GGUFStitcher(str(world["db"]), str(tmp_path / "gguf_config.txt"), str(flipped), world["files"]["Q4_K"])
    with pytest.raises(gguf_stitcher.StitchError, match=r"verify: tensor 'blk\.1\.attn_v\.weight'"):
        st.verify("cuda")
    # the command: --verify-only checks the file that is there, names the tensor on stderr and exits non-zero
    capsys.readouterr()
    assert gguf_stitcher.main([str(world["db"]), str(flipped)] + argv[2:] + ["--verify-only"]) == 1
    assert "verify: tensor 'blk.1.attn_v.weight'" in capsys.readouterr().err
    assert gguf_stitcher.main([str(world["db"]), world["out"]] + argv[2:] + ["--verify-only"]) == 0
    good = gguf_stitcher.GGUFStitcher(str(world["db"]), str(tmp_path / "gguf_config.txt"), world["out"], world["files"]["Q4_K"])
    assert good.verify("cuda") == 21
