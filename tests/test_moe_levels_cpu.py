"""The one-pass level build on a fused-expert model, host side on the CPU: the opt-in flag and its refusal, and
Quantizer.quantize_levels(fused_experts=True, level_db=...) on the tiny Mixtral of tests/test_moe_quantize_cpu.py (2 layers,
E = 5 with never-routed experts, H = 256, I = 512) with the compute backend replaced by tests/fake_ops.py plus an oracle-backed
band walk and a pack_bands restated band by band: trees under the checkpoint's names, the propagated level equal to an
ordinary run, never-routed experts equal to RTN, the database equal to converting and splitting the trees, a hole in a unit."""
import json
import os
import sys
from pathlib import Path

import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEVELS = ("Q2_K", "Q4_K", "Q6_K")
OFFSET_KEYS = ("data_offset", "data_offset_original")


def _strip(d):
    return {k: v for k, v in d.items() if k not in OFFSET_KEYS}


# ------------------------------------------------------------------------------------------------ the CLI
def _args(tmp_path, extra):
    from gptq_gguf_toolkit_amd import quant
    calib = tmp_path / "calib.pt"
    if not calib.exists():
        torch.save([torch.zeros(1, 8, dtype=torch.long)], str(calib))
    return quant.parse_args(["--model_name_or_path", "m", "--calibration_data", str(calib), "--save_dir", str(tmp_path / "out"),
                             "--quantizable_modules", r"experts\.\d+\.w[123]$", "--pre_block_modules", "model.embed_tokens",
                             "--block_modules", "model.layers"] + extra)


def test_level_fused_experts_flag_and_its_refusal(tmp_path, capsys, monkeypatch):
    """Fails without the feature: the flag does not exist."""
    from gptq_gguf_toolkit_amd.quant import levels_problem
    monkeypatch.setenv("WORLD_SIZE", "1")
    a = _args(tmp_path, ["--levels", "Q2_K", "Q4_K", "--propagate_level", "Q4_K", "--level_fused_experts"])
    assert a.level_fused_experts is True and a.levels == ["Q2_K", "Q4_K"]
    assert _args(tmp_path, ["--levels", "Q2_K", "--propagate_level", "none"]).level_fused_experts is False
    assert _args(tmp_path, []).level_fused_experts is False
    with pytest.raises(SystemExit):
        _args(tmp_path, ["--level_fused_experts"])
    assert "--level_fused_experts needs --levels" in capsys.readouterr().err
    import types
    ns = types.SimpleNamespace(levels=None, propagate_level=None, level_db=None, level_fused_experts=True,
                               bit_width_configuration=None, act_order=False, static_groups=False)
    assert levels_problem(ns) == "--level_fused_experts needs --levels: it is an option of the one-pass level build"
    ns.level_fused_experts = False
    assert levels_problem(ns) is None
    ns.levels, ns.propagate_level, ns.level_fused_experts = ["Q4_K"], "Q4_K", True
    assert levels_problem(ns, world_size=1) is None
    import inspect
    from gptq_gguf_toolkit_amd.quantizer import Quantizer
    assert inspect.signature(Quantizer.quantize_levels).parameters["fused_experts"].default is False


# ------------------------------------------------------------------------------------------------ the backend
def _backend(monkeypatch):
    import fake_ops
    from test_levels_cpu import _fake_bands
    from gptq_gguf_toolkit_amd import packing_utils
    fake = fake_ops.install(monkeypatch)
    inner, calls = _fake_bands(fake)

    side = {}  # id(stacked qweight) -> the per-band results behind it

    def gptq_quantize_bands(W, U, bands, *a, return_stacked=False, **k):
        res = inner(W, U, bands, *a, **k)
        if not return_stacked:
            return res
        # what the real op returns: five stacked buffers (qweight [R, C], d, s, dmin, m; s / m as the bytes of the bands one
        # after the other); the restated pack_bands below finds a band's own arrays through `side`
        flat = lambda i: torch.cat([r[i].contiguous().view(torch.uint8).reshape(-1) for r in res])  # noqa: E731
        q = torch.cat([r[0].contiguous().view(torch.uint8) for r in res])
        stacked = (q, torch.cat([r[1] for r in res]), flat(2), torch.cat([r[3] for r in res]), flat(4))
        side[id(q)] = (q, res)
        return res, stacked

    def pack_bands(results, bands, outs=None, row_srcs=None):
        """ops.pack_bands restated band by band: outs[k] = pack(q_type_k, *band k)."""
        if len(results) == 5 and all(torch.is_tensor(t) for t in results):  # the stacked buffers of one walk
            results = side.pop(id(results[0]))[1]
        assert len(bands) == len(results) and (outs is None or len(outs) == len(bands))
        views = []
        for k, ((_, t), five) in enumerate(zip(bands, results)):
            if row_srcs is not None and row_srcs[k] is not None:  # output row r is packed from band row row_srcs[k][r]
                five = [x[row_srcs[k].long()] for x in five]
            packed = fake.pack(int(t), *five)
            out = outs[k] if outs is not None else torch.empty(packed.numel(), dtype=torch.uint8)  # (None: allocated here)
            assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == packed.numel()
            out.copy_(packed.reshape(-1))
            views.append(out.view(packed.shape))
        return views

    monkeypatch.setattr(fake, "gptq_quantize_bands", gptq_quantize_bands, raising=False)
    monkeypatch.setattr(fake, "pack_bands", pack_bands, raising=False)
    monkeypatch.setattr(fake, "BANDS_MAX", 64, raising=False)
    monkeypatch.setattr(packing_utils, "_ops", fake)  # the converter's packer: the oracle's bit-packer stands in
    monkeypatch.setattr(packing_utils, "_dev", lambda t: t.contiguous())
    return fake, calls


from tiny_moe import MOE_REGEX  # noqa: E402  (the four attention projections and every expert matrix)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """ONE quantize_levels(fused_experts=True, level_db=DB) on the tiny Mixtral, an ordinary all-Q4_K quantize() next to it,
    and convert + split of the three trees."""
    from test_moe_quantize_cpu import make_quantizer, tiny_mixtral
    from gptq_gguf_toolkit_amd import gguf_splitter
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import convert
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    mp = pytest.MonkeyPatch()
    try:
        fake, calls = _backend(mp)
        tmp = tmp_path_factory.mktemp("moe_levels")
        model = tiny_mixtral()
        hf = tmp / "hf"
        model.save_pretrained(str(hf), safe_serialization=True)
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        experts = [layer.mlp.experts for layer in model.model.layers]
        os.makedirs(tmp / "lv")
        q = make_quantizer(model, tmp / "lv", regex=MOE_REGEX)
        q.quant_non_block_modules = False
        q.quantize_levels([T[n] for n in LEVELS], T.Q4_K, fused_experts=True, level_db=str(tmp / "db"), level_db_model=str(hf),
                          level_db_vocab=False)
        assert all(layer.mlp.experts is m for layer, m in zip(model.model.layers, experts))  # restored, by identity
        ordinary = tiny_mixtral()
        os.makedirs(tmp / "q4")
        o = make_quantizer(ordinary, tmp / "q4", regex=MOE_REGEX)
        o.quant_non_block_modules = False
        o.quantize({k: T.Q4_K for k in ("w1", "w2", "w3", "q_proj", "k_proj", "v_proj", "o_proj")})
        for n in LEVELS:
            out = convert(Path(hf), tmp / "lv" / n, tmp / f"{n}.gguf", "f16", vocab=False)
            gguf_splitter.main([str(out), str(tmp / "split"), "--gguf-layers", "--exact"])
    finally:
        mp.undo()
    return dict(tmp=tmp, model=model, before=before, ordinary=ordinary, calls=calls)


def _tree(d, name):
    x = torch.load(os.path.join(d, name, "data.pth"), weights_only=True)
    return x, [x["qweight"], x["super_group_scale"], x["group_scale_quant"], x["super_group_zero"], x["group_zero_quant"]]


def test_trees_under_the_checkpoints_names_and_the_propagated_level_is_the_ordinary_run(built):
    """Fails without the feature: quantize_levels has no fused_experts keyword (TypeError)."""
    import fake_ops
    from test_moe_quantize_cpu import E5, H, I, LAYERS
    tmp, model = built["tmp"], built["model"]
    names = sorted([f"model.layers.{i}.block_sparse_moe.experts.{e}.w{k}" for i in range(LAYERS) for e in range(E5) for k in (1, 2, 3)]
                   + [f"model.layers.{i}.self_attn.{p}_proj" for i in range(LAYERS) for p in "qkvo"])
    for n in LEVELS:
        assert sorted(os.listdir(tmp / "lv" / n)) == names
    # the Q4_K tree and the model afterwards: an ordinary quantize() of all-Q4_K, bit for bit
    assert sorted(os.listdir(tmp / "q4")) == names
    for name in names:
        a, b = _tree(tmp / "lv" / "Q4_K", name)[0], _tree(tmp / "q4", name)[0]
        assert set(a) == set(b)
        for k in a:
            assert (a[k] == b[k]) if k == "q_type" else (a[k].dtype == b[k].dtype and torch.equal(a[k], b[k])), (name, k)
    for (n, p), (n2, p2) in zip(sorted(model.named_parameters()), sorted(built["ordinary"].named_parameters())):
        assert n == n2 and torch.equal(p, p2), n
    # the fused parameters hold the Q4_K level's dequantized weights, slice by slice
    qid = {"Q2_K": 10, "Q4_K": 12, "Q6_K": 14}
    for i in range(LAYERS):
        ex = model.model.layers[i].mlp.experts
        routed = set()
        for e in range(E5):
            for r, rows in (("w1", slice(0, I)), ("w3", slice(I, 2 * I)), ("w2", None)):
                name = f"model.layers.{i}.block_sparse_moe.experts.{e}.{r}"
                d, five = _tree(tmp / "lv" / "Q4_K", name)
                have = ex.down_proj[e] if r == "w2" else ex.gate_up_proj[e, rows]
                assert torch.equal(have.detach(), fake_ops.dequantize(12, *five, out_dtype=torch.float32)), name
                key = f"model.layers.{i}.mlp.experts." + ("down_proj" if r == "w2" else "gate_up_proj")
                w0 = built["before"][key][e] if r == "w2" else built["before"][key][e, rows]
                # an expert no calibration token reaches: H = I, round-to-nearest of its weights at EVERY level
                same = []
                for n in LEVELS:
                    d, five = _tree(tmp / "lv" / n, name)
                    assert d["q_type"] == qid[n] and tuple(d["qweight"].shape) == ((H, I) if r == "w2" else (I, H))
                    rtn = fake_ops.rtn_quantize(w0.contiguous(), qid[n])
                    same.append(all(torch.equal(a, b) for a, b in zip(five, rtn)))
                if e == E5 - 1:
                    assert all(same), name
                elif not all(same):
                    routed.add(e)
        assert routed and E5 - 1 not in routed  # the walk did more than round: error feedback reached the routed experts


def test_database_equals_convert_and_split_of_the_trees(built):
    """Fails without the feature: the sink refuses MixtralForCausalLM."""
    from test_moe_quantize_cpu import E5, H, I, LAYERS
    from gptq_gguf_toolkit_amd import level_db
    split, db = built["tmp"] / "split", built["tmp"] / "db"
    assert not os.path.exists(str(db) + ".partial")
    files = sorted(os.path.relpath(os.path.join(d, f), split) for d, _, fs in os.walk(split) for f in fs)
    assert files == sorted(os.path.relpath(os.path.join(d, f), db) for d, _, fs in os.walk(db) for f in fs)
    units = [f"blk.{i}.ffn_{r}_exps.weight" for i in range(LAYERS) for r in ("gate", "up", "down")]
    for u in units:
        assert sum(f.startswith(u + os.sep) and f.endswith(".pth") for f in files) == len(LEVELS)
    for f in files:
        a, b = open(split / f, "rb").read(), open(db / f, "rb").read()
        if f.endswith(".pth"):
            assert a == b, f
        elif f.endswith("-metadata.json"):
            ja, jb = json.loads(a)["tensor_info"], json.loads(b)["tensor_info"]
            assert set(ja) - set(jb) == {"data_offset_original"} and list(_strip(ja).items()) == list(jb.items()), f
    ma, mb = json.load(open(split / "manifest.json")), json.load(open(db / "manifest.json"))
    assert ma["metadata"] == mb["metadata"] and list(ma["metadata"]) == list(mb["metadata"])
    assert list(ma["layers"]) == list(mb["layers"])  # tensor order: a unit stands where its last expert's tensor stood
    for name in ma["layers"]:  # the split's manifest holds what its last run left; the writer's lists every level
        la, lb = ma["layers"][name], mb["layers"][name]
        assert {k: v for k, v in la.items() if k != "bitwidths"} == {k: v for k, v in lb.items() if k != "bitwidths"}
        for bw in la["bitwidths"]:
            assert list(_strip(la["bitwidths"][bw]).items()) == list(lb["bitwidths"][bw].items()), (name, bw)
    assert list(mb["layers"]["blk.0.ffn_gate_exps.weight"]["bitwidths"]) == ["2.5625", "4.5", "6.5625"]
    da, dbj = json.load(open(split / "gguf_layer_database.json")), json.load(open(db / "gguf_layer_database.json"))
    assert list(da) == list(dbj)
    for name in da:
        assert list(_strip(da[name]).items()) == list(dbj[name].items()), name
    # a unit level is [E, R, C]: 3-D sidecar, and the size the sidecar describes
    for i in range(LAYERS):
        for role, shape in (("gate", (E5, I, H)), ("up", (E5, I, H)), ("down", (E5, H, I))):
            ldir = level_db.layer_dir(str(db), f"model.layers.{i}.mlp.experts.{role}_proj")
            assert ldir.endswith(f"blk.{i}.ffn_{role}_exps.weight") and len(level_db.level_files(ldir)) == len(LEVELS)
            for f in level_db.level_files(ldir):
                rec = level_db.read_sidecar(os.path.join(ldir, f))
                assert rec.shape == shape and rec.np_shape[:2] == [E5, shape[1]]
                level_db.check_level_size(rec)
    # the router and the norms, which GPTQ does not touch, are there as the packer writes them (compared above, byte for byte)
    assert "blk.0.ffn_gate_inp.weight" in mb["layers"] and "blk.0.attn_q.weight" in mb["layers"]


def test_a_hole_in_a_unit_raises_and_leaves_no_database(tmp_path, monkeypatch):
    from test_moe_quantize_cpu import make_quantizer, tiny_mixtral
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    _backend(monkeypatch)
    model = tiny_mixtral()
    experts = [layer.mlp.experts for layer in model.model.layers]
    model.save_pretrained(str(tmp_path / "hf"), safe_serialization=True)
    os.makedirs(tmp_path / "lv")
    # a regex that leaves expert 3 out: slot 3 of every unit is never filled
    q = make_quantizer(model, tmp_path / "lv", regex=r".*layers.*experts\.[0124]\.w[123]$")
    q.quant_non_block_modules = False
    with pytest.raises(RuntimeError, match=r"blk\.0\.ffn_.*slots \[3\] of 5 were never filled"):
        q.quantize_levels([T.Q2_K, T.Q4_K], T.Q4_K, fused_experts=True, level_db=str(tmp_path / "db"),
                          level_db_model=str(tmp_path / "hf"), level_db_vocab=False)
    assert not os.path.exists(tmp_path / "db") and not os.path.exists(str(tmp_path / "db") + ".partial")
    assert all(layer.mlp.experts is m for layer, m in zip(model.model.layers, experts))  # the model has its own modules back


def test_default_keeps_the_refusal_and_other_refusals_stand(tmp_path, monkeypatch):
    from test_moe_quantize_cpu import make_quantizer, tiny_mixtral
    _backend(monkeypatch)
    model = tiny_mixtral()
    with pytest.raises(NotImplementedError, match=r"quantize_levels: model\.layers\.0\.mlp\.experts.*fused_experts=True"):
        make_quantizer(model, tmp_path).quantize_levels([12], 12)
    gelu = tiny_mixtral(hidden_act="gelu")
    with pytest.raises(NotImplementedError, match=r"model\.layers\.0\.mlp\.experts.*activation"):
        make_quantizer(gelu, tmp_path).quantize_levels([12], 12, fused_experts=True)
    q = make_quantizer(model, tmp_path)
    q.quantizer_kwargs["act_order"] = True
    with pytest.raises(ValueError, match="act_order"):
        q.quantize_levels([12], 12, fused_experts=True)


def test_coarser_levels_hurt_more_per_unit_in_fp64(built):
    """The check tests/test_gpu_moe_levels.py's per-unit ordering rests on: on the oracle-backed database of this model (the
    trees hold the same numbers as the database, byte for byte above) the unit errors in fp64 fall Q2_K > Q4_K > Q6_K for
    every unit, with the estimator's common-scale Hessians from the unmodified model's calibration inputs."""
    import fake_ops
    from test_moe_errest_cpu import _captured_expert_inputs, _want_unit_error
    from test_moe_quantize_cpu import E5, I, LAYERS, calib, tiny_mixtral
    model = tiny_mixtral()
    data = [([], {"input_ids": ids}) for ids in calib()]
    acts, n_tokens = _captured_expert_inputs(model, data)
    qid = {"Q2_K": 10, "Q4_K": 12, "Q6_K": 14}
    for i in range(LAYERS):
        ex = model.model.layers[i].mlp.experts
        for role, r, W, xs in (("gate", "w1", ex.gate_up_proj.detach()[:, :I], acts[f"model.layers.{i}.mlp.experts"][0]),
                               ("up", "w3", ex.gate_up_proj.detach()[:, I:], acts[f"model.layers.{i}.mlp.experts"][0]),
                               ("down", "w2", ex.down_proj.detach(), acts[f"model.layers.{i}.mlp.experts"][1])):
            errs = []
            for n in LEVELS:
                W_c = torch.stack([fake_ops.dequantize(qid[n], *_tree(built["tmp"] / "lv" / n,
                                                                      f"model.layers.{i}.block_sparse_moe.experts.{e}.{r}")[1])
                                   for e in range(E5)])
                errs.append(_want_unit_error(W, xs, n_tokens, W_c))
            print(f"layer {i} {role}: " + "  ".join(f"{n} {v:.4e}" for n, v in zip(LEVELS, errs)))
            assert errs[0] > errs[1] > errs[2] > 0, (i, role, errs)
