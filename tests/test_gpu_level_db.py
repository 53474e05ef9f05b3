"""-m gpu: the level database written straight from the one-pass level build (Quantizer.quantize_levels(level_db=...)) on the
tiny Llama, against the long way round from the SAME run's trees -- convert() per level, then gguf_splitter --gguf-layers
--exact -- byte for byte; its consumers (LevelStore, the stitcher); level_db_only; and the CLI's refusals."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

OFFSET_KEYS = ("data_offset", "data_offset_original")
STEMS = ["2.5625-Q2_K", "4.5-Q4_K", "6.5625-Q6_K"]


def _drive(root, tag, model_dir, **kw):
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    from gptq_gguf_toolkit_amd.quantizer import Quantizer
    model = tiny_llama()  # fp32
    if not os.path.isdir(model_dir):
        model.save_pretrained(model_dir)  # the untouched checkpoint: config.json + model.safetensors, no tokenizer
    model = model.cuda()
    data = [([], {"input_ids": ids}) for ids in tiny_calib()]
    os.makedirs(root / tag, exist_ok=True)
    drv = Quantizer(model, data_loader=data, quantizable_modules=r".*layers.*((q|k|v|o|gate|up|down)_proj)$",
                    quantizer_kwargs=dict(rel_damp=0.01, block_size=128, act_order=False, quant_scale="absmax",
                                          static_groups=False, rmin=-1.0, rdelta=0.1, nstep=20, verbose=False),
                    pre_block_modules=["model.embed_tokens"], block_modules="model.layers",
                    post_block_modules=["lm_head"], quant_non_block_modules=False, device="cuda:0", save_dir=str(root / tag))
    drv.quantize_levels([T.Q2_K, T.Q4_K, T.Q6_K], T.Q4_K, level_db=str(root / f"db_{tag}"), level_db_model=str(model_dir),
                        level_db_vocab=False, **kw)
    torch.cuda.synchronize()
    return model


def _level_files(db):
    return sorted(os.path.relpath(os.path.join(d, f), db) for d, _, fs in os.walk(db) for f in fs if f.endswith(".pth"))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """ONE level build that writes the trees and the database DB; DB2 from those trees by convert() + split per level; the
    same build twice more without trees (the second one measures what two runs give each other)."""
    from gptq_gguf_toolkit_amd import gguf_splitter
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import convert
    root = tmp_path_factory.mktemp("level_db_gpu")
    keep = os.environ.get("GQ_SAVE_SLOT_MB")
    os.environ["GQ_SAVE_SLOT_MB"] = "8"  # the tiny model's files: no 704 MB staging slots to pin per run
    try:
        model_dir = root / "model"
        w = {"root": root, "model": _drive(root, "a", model_dir), "db": root / "db_a", "db2": root / "db2", "gguf": {}}
        for lv in ("Q2_K", "Q4_K", "Q6_K"):  # the order of --levels: the last split leaves its records in the manifests
            w["gguf"][lv] = str(root / f"{lv}.gguf")
            convert(Path(model_dir), root / "a" / lv, Path(w["gguf"][lv]), vocab=False)
            gguf_splitter.main([w["gguf"][lv], str(w["db2"]), "--gguf-layers", "--exact"])
        _drive(root, "b", model_dir, trees=False)
        _drive(root, "c", model_dir, trees=False)
    finally:
        if keep is None:
            os.environ.pop("GQ_SAVE_SLOT_MB", None)
        else:
            os.environ["GQ_SAVE_SLOT_MB"] = keep
    return w


def test_database_equals_convert_and_split_of_the_same_runs_trees(world):
    db, db2 = world["db"], world["db2"]
    files = _level_files(db2)
    assert len(files) == 14 * 3 + 5 + 2  # 14 Linears at three levels, five norms, token_embd and output
    assert files == _level_files(db)
    for f in files:
        a, b = np.fromfile(db2 / f, np.uint8), np.fromfile(db / f, np.uint8)
        what = "the q / k row gather" if ("attn_q" in f or "attn_k" in f) else "the packed bytes"
        assert a.size == b.size and np.array_equal(a, b), f"{f}: {what} differ in {(a != b).mean():.4%} of the bytes"
        sa = json.load(open(str(db2 / f)[:-4] + "-metadata.json"))["tensor_info"]
        sb = json.load(open(str(db / f)[:-4] + "-metadata.json"))["tensor_info"]
        assert {k: v for k, v in sa.items() if k not in OFFSET_KEYS} == sb, f
    ma, mb = json.load(open(db2 / "manifest.json")), json.load(open(db / "manifest.json"))
    assert ma["metadata"] == mb["metadata"] and list(ma["metadata"]) == list(mb["metadata"])
    assert list(ma["layers"]) == list(mb["layers"])
    assert list(mb["layers"]["blk.0.attn_q.weight"]["bitwidths"]) == ["2.5625", "4.5", "6.5625"]  # all levels, not the last
    da, dbj = json.load(open(db2 / "gguf_layer_database.json")), json.load(open(db / "gguf_layer_database.json"))
    assert list(da) == list(dbj)
    for name in da:  # the last level's record, as the last split leaves it
        assert {k: v for k, v in da[name].items() if k not in OFFSET_KEYS} == dbj[name], name
    assert not os.path.exists(str(db) + ".partial")


def test_consumers_read_the_written_database(world, tmp_path):
    import copy
    from gptq_gguf_toolkit_amd import evo_quant_search as S
    from gptq_gguf_toolkit_amd.gguf_stitcher import stitch_search_result
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    db, db2 = world["db"], world["db2"]
    after = world["model"]  # holds the propagated level's dequantized weights, in the weight dtype (fp32)
    model = copy.deepcopy(after)
    names = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and "layers" in n]
    assert len(names) == 14
    with torch.no_grad():
        for n in names:
            model.get_submodule(n).weight.zero_()
    store = LevelStore(model, str(db), "cuda", names)
    assert all(store.level_keys(n) == [2.5625, 4.5, 6.5625] for n in names)
    assert store.switch({n: 4.5 for n in names}) == 14
    for n in names:  # one rounding either side: the block decoder and the driver's dequantize compute d * s * q - dmin * m in fp32
        assert torch.equal(model.get_submodule(n).weight, after.get_submodule(n).weight), n
    # a mixed assignment: all three levels, q and k of block 0 on different ones
    widths = [2.5625, 4.5, 6.5625]
    assignment = {n: widths[(i + i // 7) % 3] for i, n in enumerate(names)}
    assignment["model.layers.0.self_attn.k_proj"] = 6.5625
    levels = S.scan_available_bitwidths(str(db), names)
    assert all([f for _, f in levels[n]] == [s + ".pth" for s in STEMS] for n in names)
    cfg = tmp_path / S.configuration_name("kl", 4.5)
    cfg.write_text(S.configuration_text([names], [[assignment[n] for n in names]], levels))
    out = stitch_search_result(str(db), str(cfg), str(tmp_path / "mixed.gguf"), verify=True)  # no original_model: the manifest's
    out2 = stitch_search_result(str(db2), str(cfg), str(tmp_path / "mixed2.gguf"), original_model=world["gguf"]["Q6_K"])
    assert open(out, "rb").read() == open(out2, "rb").read()


def test_level_db_only_writes_the_same_database_and_no_trees(world):
    root = world["root"]
    assert sorted(os.listdir(root / "a")) == ["Q2_K", "Q4_K", "Q6_K"]
    for tag in ("b", "c"):
        assert os.listdir(root / tag) == [], tag
    files = _level_files(world["db"])
    assert files == _level_files(root / "db_b") == _level_files(root / "db_c")

    def rate(x, y, f):
        a, b = np.fromfile(x / f, np.uint8), np.fromfile(y / f, np.uint8)
        assert a.size == b.size, f
        return float((a != b).mean())

    # what two ordinary runs of the same build give each other (b against c), file by file: the bound for a against b
    for f in files:
        own, got = rate(root / "db_b", root / "db_c", f), rate(world["db"], root / "db_b", f)
        if own or got:
            print(f"    {f}: with trees vs without {got:.4%}   without vs without {own:.4%}")
        assert got <= own, f
    ma, mb = json.load(open(world["db"] / "manifest.json")), json.load(open(root / "db_b" / "manifest.json"))
    assert ma["metadata"] == mb["metadata"] and ma["layers"] == mb["layers"]


@pytest.mark.parametrize("flags,message", [
    (["--level_db", "DB"], "--level_db needs --levels"),
    (["--levels", "Q2_K", "Q4_K", "--propagate_level", "Q4_K", "--level_db", "DB", "--act_order"], "--act_order / --static_groups"),
    (["--levels", "Q2_K", "Q4_K", "--propagate_level", "Q4_K", "--level_db_only"], "--level_db_only needs --level_db"),
    (["--levels", "Q2_K", "Q4_K", "--propagate_level", "Q4_K", "--level_db", "DB"], "local directory"),
])
def test_cli_refuses_before_any_work(tmp_path, flags, message):
    """The calibration file does not exist: a run that got as far as loading it would say so instead."""
    flags = [str(tmp_path / "db") if f == "DB" else f for f in flags]
    cmd = [sys.executable, os.path.join(ROOT, "gptq-gguf-toolkit_amd", "quant.py"), "--model_name_or_path", "no-such/model",
           "--quantizable_modules", ".*", "--pre_block_modules", "model.embed_tokens", "--block_modules", "model.layers",
           "--calibration_data", str(tmp_path / "missing.pt"), "--save_dir", str(tmp_path / "out")] + flags
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "db").exists() and not (tmp_path / "out").exists()
