"""-m gpu: the one-pass level build of a fused-expert model on the device, and the chain behind it: the tiny Mixtral of
tests/test_moe_quantize_cpu.py (2 layers, E = 5 with never-routed experts, H = 256, I = 512, fp32) through
Quantizer.quantize_levels(fused_experts=True, level_db=...) -> database with stacked expert units -> LevelStore -> search ->
stitch, and the estimator on that database."""
import io
import json
import os
import sys
from contextlib import redirect_stdout
from pathlib import Path

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEVELS = ("Q2_K", "Q4_K", "Q6_K")
OFFSET_KEYS = ("data_offset", "data_offset_original")
REGEX = r".*layers.*((q|k|v|o|gate|up|down)_proj)$"  # the estimator CLI's default
PRE = ["model.embed_tokens", "model.rotary_emb"]
ROLES = (("gate", "w1"), ("up", "w3"), ("down", "w2"))


def _build(root, tag, hf, **kw):
    from test_moe_quantize_cpu import make_quantizer, tiny_mixtral
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    model = tiny_mixtral().cuda()
    os.makedirs(root / tag, exist_ok=True)
    q = make_quantizer(model, root / tag, device="cuda:0")
    q.quant_non_block_modules = False
    q.quantize_levels([T[n] for n in LEVELS], T.Q4_K, fused_experts=True, level_db=str(root / f"db_{tag}"), level_db_model=str(hf),
                      level_db_vocab=False, **kw)
    torch.cuda.synchronize()
    return model


def _level_files(db):
    return sorted(os.path.relpath(os.path.join(d, f), db) for d, _, fs in os.walk(db) for f in fs if f.endswith(".pth"))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """Build "a": trees + database with the Q8_0 level and the unweighted round-to-nearest IQ4_XS level; DB2 from a's trees by
    convert() + split per level; build "g": the database alone with the IQ4_XS level from GPTQ's walk."""
    from test_moe_quantize_cpu import calib, tiny_mixtral
    from gptq_gguf_toolkit_amd import gguf_splitter
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import convert
    root = tmp_path_factory.mktemp("moe_levels_gpu")
    keep = os.environ.get("GQ_SAVE_SLOT_MB")
    os.environ["GQ_SAVE_SLOT_MB"] = "8"  # the tiny model's files: no 704 MB staging slots to pin per run
    try:
        hf = root / "hf"
        tiny_mixtral().save_pretrained(str(hf), safe_serialization=True)
        w = {"root": root, "hf": hf, "db": root / "db_a", "db2": root / "db2", "dbg": root / "db_g", "gguf": {}}
        w["model"] = _build(root, "a", hf, level_db_q8_0=True, level_db_iq4=("IQ4_XS",), level_db_iq4_importance="none")
        for lv in LEVELS:  # the order of --levels: the last split leaves its records in the manifests
            w["gguf"][lv] = str(root / f"{lv}.gguf")
            convert(Path(hf), root / "a" / lv, Path(w["gguf"][lv]), vocab=False)
            gguf_splitter.main([w["gguf"][lv], str(w["db2"]), "--gguf-layers", "--exact"])
        _build(root, "g", hf, trees=False, level_db_iq4=("IQ4_XS",), level_db_iq4_method="gptq")
    finally:
        if keep is None:
            os.environ.pop("GQ_SAVE_SLOT_MB", None)
        else:
            os.environ["GQ_SAVE_SLOT_MB"] = keep
    w["data"] = [([], {"input_ids": ids}) for ids in calib()]
    return w


def _units(layers=2):
    return [f"model.layers.{i}.mlp.experts.{r}_proj" for i in range(layers) for r, _ in ROLES]


def _stacked_checkpoint(w, i, role):
    """The checkpoint's [E, R, C] weights of a unit: the unmodified model's fused parameter, per expert as the packer reads them."""
    from test_moe_quantize_cpu import I, tiny_mixtral
    if "fresh" not in w:
        w["fresh"] = tiny_mixtral().cuda()
    ex = w["fresh"].model.layers[i].mlp.experts
    return {"gate": ex.gate_up_proj.detach()[:, :I], "up": ex.gate_up_proj.detach()[:, I:], "down": ex.down_proj.detach()}[role].contiguous()


def test_database_equals_convert_and_split_of_the_same_runs_trees(world):
    """Fails without the feature: quantize_levels has no fused_experts keyword, the sink refuses MixtralForCausalLM."""
    db, db2 = world["db"], world["db2"]
    extra = ("8.5-Q8_0.pth", "4.25-IQ4_XS.pth")
    files = [f for f in _level_files(db) if not f.endswith(extra)]
    assert files == _level_files(db2)
    assert sum("_exps.weight" in f for f in files) == 2 * 3 * len(LEVELS)
    for f in files:
        a, b = np.fromfile(db2 / f, np.uint8), np.fromfile(db / f, np.uint8)
        assert a.size == b.size and np.array_equal(a, b), f"{f}: the bytes differ in {(a != b).mean():.4%}"
        sa = json.load(open(str(db2 / f)[:-4] + "-metadata.json"))["tensor_info"]
        sb = json.load(open(str(db / f)[:-4] + "-metadata.json"))["tensor_info"]
        assert {k: v for k, v in sa.items() if k not in OFFSET_KEYS} == sb, f
    ma, mb = json.load(open(db2 / "manifest.json")), json.load(open(db / "manifest.json"))
    assert ma["metadata"] == mb["metadata"] and list(ma["metadata"]) == list(mb["metadata"])
    assert list(ma["layers"]) == list(mb["layers"])
    # IQ4 before the K-quant levels, Q8_0 after
    assert list(mb["layers"]["blk.0.ffn_up_exps.weight"]["bitwidths"]) == ["4.25", "2.5625", "4.5", "6.5625", "8.5"]
    da, dbj = json.load(open(db2 / "gguf_layer_database.json")), json.load(open(db / "gguf_layer_database.json"))
    assert list(da) == list(dbj)
    for name in da:  # as for dense tensors: the last registered level is the record -- Q8_0 where there is one, never IQ4
        if "8.5" in mb["layers"][name]["bitwidths"]:
            assert dbj[name]["quantization"] == "Q8_0" and ("_exps." in name or "attn_" in name), name
        else:
            assert {k: v for k, v in da[name].items() if k not in OFFSET_KEYS} == dbj[name], name
    dg = json.load(open(world["dbg"] / "gguf_layer_database.json"))  # without Q8_0: the last K-quant level, IQ4 came first
    assert all(dg[f"blk.{i}.ffn_{r}_exps.weight"]["quantization"] == "Q6_K" for i in range(2) for r, _ in ROLES)
    assert not os.path.exists(str(db) + ".partial")


def test_q8_0_and_iq4_levels_of_a_unit_are_the_encoders_of_the_stacked_checkpoint(world):
    from test_moe_quantize_cpu import E5
    from gptq_gguf_toolkit_amd import level_db, ops
    for i in range(2):
        for role, _ in ROLES:
            x = _stacked_checkpoint(world, i, role)
            flat = x.view(-1, x.shape[-1]).contiguous()
            d = world["db"] / f"blk.{i}.ffn_{role}_exps.weight"
            for f, want in (("8.5-Q8_0.pth", ops.quantize_q8_0(flat)), ("4.25-IQ4_XS.pth", ops.quantize_iq4(flat, 23))):
                rec = level_db.read_sidecar(str(d / f))
                level_db.check_level_size(rec)
                assert rec.shape == tuple(x.shape) and rec.np_shape[0] == E5
                got = torch.from_numpy(level_db.read_level_raw(rec)).cuda()
                assert torch.equal(got, want.view(-1)), (i, role, f)
                lv = level_db.load_level(rec.path, "cuda", str(world["db"]))
                assert tuple(lv.shape) == tuple(x.shape)  # a unit level is [E, R, C]
    # ops.quantize_iq4's out=: a slot of a stacked buffer, the same bytes
    x = _stacked_checkpoint(world, 0, "down")
    buf = torch.zeros(E5, x.shape[1], x.shape[2] // 256 * 136, dtype=torch.uint8, device="cuda")
    for e in range(E5):
        ops.quantize_iq4(x[e], 23, out=buf[e].view(-1))
    assert torch.equal(buf.view(-1, buf.shape[-1]), ops.quantize_iq4(x.view(-1, x.shape[-1]).contiguous(), 23))


def test_gptq_iq4_level_of_a_unit_exists_and_has_its_size(world):
    from gptq_gguf_toolkit_amd import level_db
    assert not os.path.exists(world["root"] / "g" / "Q4_K")  # trees=False
    for i in range(2):
        for role, _ in ROLES:
            d = world["dbg"] / f"blk.{i}.ffn_{role}_exps.weight"
            assert level_db.level_files(str(d)) == ["2.5625-Q2_K.pth", "4.25-IQ4_XS.pth", "4.5-Q4_K.pth", "6.5625-Q6_K.pth"]
            rec = level_db.read_sidecar(str(d / "4.25-IQ4_XS.pth"))
            level_db.check_level_size(rec)
            a, b = np.fromfile(d / "4.25-IQ4_XS.pth", np.uint8), np.fromfile(world["db"] / d.name / "4.25-IQ4_XS.pth", np.uint8)
            assert a.size == b.size and not np.array_equal(a, b)  # the walk's bytes, not round-to-nearest's
            for f in ("2.5625-Q2_K.pth", "4.5-Q4_K.pth", "6.5625-Q6_K.pth"):  # the K-quant levels do not depend on the IQ4 method
                assert np.array_equal(np.fromfile(d / f, np.uint8), np.fromfile(world["db"] / d.name / f, np.uint8)), (d.name, f)


def test_chain_store_switch_search_stitch(world, tmp_path):
    import copy
    from gptq_gguf_toolkit_amd import evo_quant_search as S
    from gptq_gguf_toolkit_amd.gguf_stitcher import stitch_search_result
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    after = world["model"]  # holds the propagated level's dequantized weights
    model = copy.deepcopy(after)
    attn = [f"model.layers.{i}.self_attn.{p}_proj" for i in range(2) for p in "qkvo"]
    with torch.no_grad():
        for layer in model.model.layers:
            layer.mlp.experts.gate_up_proj.zero_()
            layer.mlp.experts.down_proj.zero_()
    store = LevelStore(model, str(world["db"]), "cuda", _units() + attn)
    assert sorted(store.units) == sorted(_units())
    assert all(store.level_keys(u) == [2.5625, 4.25, 4.5, 6.5625, 8.5] for u in _units())
    assert store.switch({n: 4.5 for n in _units() + attn}) == len(_units() + attn)
    for a, b in zip(model.model.layers, after.model.layers):  # uniform Q4_K: the propagated model's fused parameters, bit for bit
        assert torch.equal(a.mlp.experts.gate_up_proj, b.mlp.experts.gate_up_proj)
        assert torch.equal(a.mlp.experts.down_proj, b.mlp.experts.down_proj)
    del store
    # one generation of the search on the database, and the result stitched and verified
    ids = [d[1]["input_ids"] for d in world["data"]]
    torch.save(ids, str(tmp_path / "ids.pt"))
    argv = ["--model_name_or_path", str(world["hf"]), "--dtype", "float32", "--attn_implementation", "eager", "--calibration_data",
            str(tmp_path / "ids.pt"), "--eval_datasets", str(tmp_path / "ids.pt"), "--calibration_tokens", "256", "--eval_tokens", "128",
            "--calibration_sequence_length", "64", "--eval_sequence_length", "64", "--generations", "1", "--offspring", "4",
            "--target_bitwidth", "5", "--quant_weights_path", str(world["db"]), "--survivors_per_selection", "2", "1",
            "--tokens_per_selection", "128", "256", "--fitness_fn", "kl", "--resident", "dense", "--seed", "33",
            "--trace_out", str(tmp_path / "trace.json")]
    with redirect_stdout(io.StringIO()):
        _, cfg = S.main(argv)
    lines = dict(line.split(": ", 1) for line in open(cfg).read().split("\n") if line)
    assert set(_units()) <= set(lines) and len(json.load(open(tmp_path / "trace.json"))) == 1
    out = stitch_search_result(str(world["db"]), str(cfg), str(tmp_path / "mixed.gguf"), verify=True)
    assert os.path.getsize(out) > 0


def test_estimator_on_the_built_database(world):
    """Per unit Q2_K > Q4_K > Q6_K: checked on the CPU in fp64 for the oracle-backed database of this model
    (tests/test_moe_levels_cpu.py::test_coarser_levels_hurt_more_per_unit_in_fp64), where it holds for every unit.  Summed over
    the units, GPTQ's IQ4_XS level must not be worse than the round-to-nearest one (importance none) of the same weights."""
    from test_moe_quantize_cpu import tiny_mixtral
    from gptq_gguf_toolkit_amd.error_estimator import ErrorEstimator
    sums = {}
    for tag, db in (("rtn", world["db"]), ("gptq", world["dbg"])):
        model = tiny_mixtral().cuda()
        est = ErrorEstimator(model, world["data"], REGEX, PRE, "model.layers", str(db), device="cuda:0")
        errors = est.estimate()[-1]
        for u in _units():
            col = {f: k for k, f in enumerate(est.levels[u])}
            e = errors[u]
            assert e[col["2.5625-Q2_K.pth"]] > e[col["4.5-Q4_K.pth"]] > e[col["6.5625-Q6_K.pth"]] > 0, (tag, u, e)
            sums[tag] = sums.get(tag, 0.0) + e[col["4.25-IQ4_XS.pth"]]
    print(f"IQ4_XS summed over the {len(_units())} units: round-to-nearest {sums['rtn']:.6e}, GPTQ {sums['gptq']:.6e}")
    assert sums["gptq"] <= sums["rtn"]
