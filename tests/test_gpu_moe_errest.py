"""-m gpu: the error estimator on the expert units of a fused-expert Mixtral (tests/moe_gguf.py's: 2 layers, E = 4, top-2,
H = 256, I = 512, fp16, random routing, so the experts see different numbers of tokens) over the RTN level database of
tests/moe_level_db.py.

Accuracy rule (tests/test_gpu_errest.py's): the anchor is the expression in fp64 torch, from inputs captured by pre-hooks on a
second CalibExperts in "loop" mode; over the case set the estimator's largest relative error must stay within 4 x the largest
relative error of torch's own fp32 evaluation of the same expression, measured here with TF32 off."""
import os
import sys

import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

LEVELS = ("Q2_K", "IQ4_XS", "Q4_K", "Q6_K")
REGEX = r".*layers.*((q|k|v|o|gate|up|down)_proj)$"  # the CLI's default
PRE = ["model.embed_tokens", "model.rotary_emb"]


def _fix(H):
    H = H.clone()
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    return H


def _quad(A, H, B, dt):
    D = (A.float() - B.float()).to(dt) if B is not None else A.to(dt)
    return ((D @ _fix(H).to(dt)) * D).sum()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The model, its calibration data, the database, the estimator's result with the units and the captured inputs."""
    import moe_gguf
    import moe_level_db as MDB
    from make_golden_shim import tiny_calib
    from gptq_gguf_toolkit_amd import moe_calibration as mc
    from gptq_gguf_toolkit_amd.error_estimator import ErrorEstimator
    tmp = tmp_path_factory.mktemp("moe_errest")
    moe_gguf.build_hf(tmp / "hf")
    model = moe_gguf.load_hf(tmp / "hf")
    db = MDB.build(model, tmp, levels=LEVELS)["db"]
    data = [([], {"input_ids": ids}) for ids in tiny_calib(n=4, L=64, seed=31)]

    # the inputs of every expert, from hooks of the test's own on a "loop" stand-in; the model is left as it was
    acts, hooks, installed, n_tokens = {}, [], [], 0
    for i, layer in enumerate(model.model.layers):
        stand_in = mc.CalibExperts(layer.mlp.experts, "loop")
        installed.append((layer.mlp, "experts", layer.mlp.experts, f"model.layers.{i}.mlp.experts"))
        layer.mlp.experts = stand_in
        acts[i] = ({}, {})
        for e in range(stand_in.num_experts):
            for lin, d in ((stand_in.expert(e).w1, acts[i][0]), (stand_in.expert(e).w2, acts[i][1])):
                hooks.append(lin.register_forward_pre_hook(lambda m, inp, d=d, e=e: d.setdefault(e, []).append(inp[0].detach().clone())))
    with torch.no_grad():
        for _, kw in data:
            model(input_ids=kw["input_ids"].cuda())
            n_tokens += kw["input_ids"].numel()
    for h in hooks:
        h.remove()
    mc.restore(installed)

    experts = [layer.mlp.experts for layer in model.model.layers]
    est = ErrorEstimator(model, data, REGEX, PRE, "model.layers", db, device="cuda:0")
    errors = est.estimate()[-1]
    assert all(layer.mlp.experts is m for layer, m in zip(model.model.layers, experts))  # restored, by identity
    return dict(model=model, data=data, db=db, acts=acts, n_tokens=n_tokens, est=est, errors=errors, MDB=MDB)


def _unit_parts(w, name):
    """(W [E, R, C], {e: inputs}) of a unit."""
    layer, role = int(name.split(".")[2]), name.rpartition(".")[2]
    ex = w["model"].model.layers[layer].mlp.experts
    inter = ex.down_proj.shape[2]
    W = {"gate_proj": ex.gate_up_proj.detach()[:, :inter], "up_proj": ex.gate_up_proj.detach()[:, inter:],
         "down_proj": ex.down_proj.detach()}[role]
    return W, w["acts"][layer][1 if role == "down_proj" else 0]


def test_unit_errors_against_fp64(world):
    """Fails without the feature: the estimator returns no unit."""
    from gptq_gguf_toolkit_amd import level_db
    assert torch.backends.cuda.matmul.allow_tf32 is False and torch.get_float32_matmul_precision() == "highest"
    w, MDB = world, world["MDB"]
    assert sorted(w["errors"]) == sorted(MDB.UNITS + MDB.ATTENTION)
    files = sorted((MDB.level_file(n) for n in LEVELS), key=level_db.level_key)
    worst_k = worst_t = 0.0
    counts = set()
    for u in MDB.UNITS:
        assert w["est"].levels[u] == files and len(w["errors"][u]) == len(files)
        W, xs = _unit_parts(w, u)
        E, _, C = W.shape
        H64 = torch.zeros(E, C, C, dtype=torch.float64, device="cuda")
        H32 = torch.zeros(E, C, C, dtype=torch.float32, device="cuda")
        for e in range(E):
            n_e = sum(x.shape[0] for x in xs.get(e, []))
            counts.add(n_e)
            for x in xs.get(e, []):  # ONE scale for every expert: 2 / N
                H64[e] += (2.0 / w["n_tokens"]) * (x.double().T @ x.double())
                H32[e].addmm_(x.float().T, x.float(), alpha=2.0 / w["n_tokens"])
        ldir = level_db.layer_dir(w["db"], u)
        for f, got in zip(files, w["errors"][u]):
            W_c = level_db.load_level(os.path.join(ldir, f), "cuda", w["db"])
            assert tuple(W_c.shape) == tuple(W.shape)
            want = float(sum(_quad(W[e], H64[e], W_c[e], torch.float64) for e in range(E))
                         / sum(_quad(W[e], H64[e], None, torch.float64) for e in range(E)))
            t32 = float(sum(_quad(W[e], H32[e], W_c[e], torch.float32) for e in range(E))
                        / sum(_quad(W[e], H32[e], None, torch.float32) for e in range(E)))
            assert 0 < got < 1
            worst_k, worst_t = max(worst_k, abs(got - want) / want), max(worst_t, abs(t32 - want) / want)
    print(f"units: largest relative error estimator {worst_k:.3e}, torch fp32 {worst_t:.3e}; tokens per expert {sorted(counts)}")
    assert len(counts) > 2  # the experts do see different numbers of tokens: the common scale matters
    assert worst_t > 0 and worst_k <= 4 * worst_t


def test_attention_errors_are_those_of_a_run_without_units(world):
    from gptq_gguf_toolkit_amd.error_estimator import ErrorEstimator
    w = world
    est = ErrorEstimator(w["model"], w["data"], r".*layers.*((q|k|v|o)_proj)$", PRE, "model.layers", w["db"], device="cuda:0")
    alone = est.estimate()[-1]
    assert sorted(alone) == sorted(w["MDB"].ATTENTION)
    assert all(alone[n] == w["errors"][n] for n in alone)  # bit for bit: the stand-in's forward is the module's


def test_level_store_gives_the_same_values_and_numel_groups(world):
    from gptq_gguf_toolkit_amd.error_estimator import ErrorEstimator
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    w, MDB = world, world["MDB"]
    store = LevelStore(w["model"], w["db"], "cuda", MDB.UNITS + MDB.ATTENTION)
    est = ErrorEstimator(w["model"], w["data"], REGEX, PRE, "model.layers", w["db"], device="cuda:0", level_store=store)
    grouped = est.estimate(group_by_numel=True)
    assert sorted(grouped[4 * 512 * 256]) == sorted(MDB.UNITS)
    for group in grouped.values():
        for n, vals in group.items():
            assert vals == w["errors"][n], n


def test_the_per_expert_loop_of_large_experts_gives_the_same_bits(world, monkeypatch):
    import gptq_gguf_toolkit_amd.error_estimator as ee
    w = world
    monkeypatch.setattr(ee, "GROUPED_MAX_TILES_PER_EXPERT", 0)  # every unit through ops.quad_form, expert by expert
    est = ee.ErrorEstimator(w["model"], w["data"], r"experts\.(gate|up|down)_proj$", PRE, "model.layers", w["db"], device="cuda:0")
    looped = est.estimate()[-1]
    assert sorted(looped) == sorted(w["MDB"].UNITS) and all(looped[u] == w["errors"][u] for u in looped)


def test_sum_over_experts_is_the_ascending_sum(world):
    """sum-of-[E] on the device against the ascending host sum, within E * 2^-53 relative."""
    from gptq_gguf_toolkit_amd import ops
    W, _ = _unit_parts(world, world["MDB"].UNITS[0])
    E, _, C = W.shape
    g = torch.Generator(device="cuda").manual_seed(3)
    X = torch.randn(E, 2 * C, C, generator=g, device="cuda").half()
    H = torch.zeros(E, C, C, device="cuda")
    for e in range(E):
        ops.h_accumulate(H[e], X[e, :C + 64 * e].contiguous(), 1.0, 2.0 / (8 * C))
    per = ops.quad_form_experts(W, H)
    host = 0.0
    for v in per.tolist():
        host += v
    assert abs(per.sum().item() - host) <= E * 2.0 ** -53 * host


def test_coarser_levels_hurt_more_summed_over_units(world):
    """Round-to-nearest levels of one weight: each step Q2_K -> Q4_K -> Q6_K shrinks the quantization step by about 4x, the
    error by about 16x, whatever positive semi-definite H weighs it.  Asserted on the sum over the units (per unit it is
    printed): a level file read for the wrong unit, or a numerator divided by another unit's denominator, breaks it."""
    w, MDB = world, world["MDB"]
    from gptq_gguf_toolkit_amd import level_db
    files = sorted((MDB.level_file(n) for n in LEVELS), key=level_db.level_key)
    col = {n: files.index(MDB.level_file(n)) for n in LEVELS}
    tot = {n: sum(w["errors"][u][col[n]] for u in MDB.UNITS) for n in LEVELS}
    for u in MDB.UNITS:
        print(u + ": " + "  ".join(f"{n} {w['errors'][u][col[n]]:.4e}" for n in LEVELS))
    print("sum over units: " + "  ".join(f"{n} {tot[n]:.4e}" for n in LEVELS))
    assert tot["Q2_K"] > tot["Q4_K"] > tot["Q6_K"] > 0
