"""-m gpu: the search evaluated from the first changed block, and on two ranks.  A Llama of 4 blocks (hidden 256, vocab 512) in
fp16 and bf16 with three RTN levels per Linear (a --gguf-layers database, as test_gpu_search.py's `world` makes them), dense
and packed residency.  The rule of every comparison: equality, unless two plain runs of the same thing differ from each other
-- then their spread is the bound (printed)."""
import copy
import json
import os
import random
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from test_suffix_cpu import llama

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

Q2, Q4, Q6 = 10, 12, 14
LEVELS = ((Q2, "2"), (Q4, "4"), (Q6, "6"))
LINEARS = r"((q|k|v|o|gate|up|down)_proj)$"
N_BLOCKS = 4


_WORLDS = {}


def make_world(name, tmp_path_factory):
    """-> dict (built once per dtype): the 4-block model on the device, its Linears, the level database, 8 calibration
    sequences of 64 tokens, the KL targets of the unmodified model (dense and top-10), and under `tmp` the checkpoint
    directory and the calibration file (for the CLI)."""
    if name in _WORLDS:
        return _WORLDS[name]
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from gptq_gguf_toolkit_amd import metrics, ops
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import map_tensor_name
    dtype = getattr(torch, name)
    tmp = tmp_path_factory.mktemp("suffix_" + name)
    model = llama(N_BLOCKS, dtype).cuda()
    names = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and re.search(LINEARS, n)]
    assert len(names) == 7 * N_BLOCKS
    for n in names:
        W = model.get_submodule(n).weight.data
        g = map_tensor_name(n + ".weight")
        (tmp / "gg" / g).mkdir(parents=True)
        for t, num in LEVELS:
            packed = ops.pack(t, *ops.rtn_quantize(W, t))
            packed.cpu().numpy().tofile(str(tmp / "gg" / g / f"{num}.pth"))
            (tmp / "gg" / g / f"{num}-metadata.json").write_text(json.dumps({"tensor_info": {
                "name": g, "type": t, "shape": [W.shape[1], W.shape[0]], "np_shape": list(packed.shape), "np_dtype": "uint8"}}))
    md = {"general.architecture": {"value": "llama"}, "llama.attention.head_count": {"value": 4},
          "llama.attention.head_count_kv": {"value": 2}}
    (tmp / "gg" / "manifest.json").write_text(json.dumps({"metadata": md}))
    g = torch.Generator().manual_seed(1)
    calib = [torch.randint(0, 512, (1, 64), generator=g) for _ in range(8)]
    torch.save(calib, str(tmp / "calib.pt"))
    model.save_pretrained(str(tmp / "hf"), safe_serialization=True)
    _WORLDS[name] = dict(model=model, names=names, db=str(tmp / "gg"), calib=calib, tmp=tmp, dtype=name,
                         kl=metrics.collect_target_logits(model, calib),
                         sparse_kl=metrics.collect_target_logits(model, calib, topk=10))
    return _WORLDS[name]


@pytest.fixture(scope="module", params=["float16", "bfloat16"])
def world(request, tmp_path_factory):
    return make_world(request.param, tmp_path_factory)


def searched(world, resident):
    """A fresh copy of the model under a level store, everything the search needs around it."""
    from gptq_gguf_toolkit_amd import evo_quant_search as S
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    model = copy.deepcopy(world["model"])
    levels = S.scan_available_bitwidths(world["db"], world["names"])
    grouped = S.group_layers(model, sorted(levels, key=S.layer_order_fn), "size")
    store = LevelStore(model, world["db"], "cuda", [n for g in grouped for n in g], resident=resident)
    store.grouped_layer_names = grouped
    ctx = S._Ctx(model, grouped, levels, S.target_bits_of(grouped, model, 4.0))
    return S, model, store, ctx


def seed_whose_first_stage_reuses(S, ctx, store, offspring, stride, world_size=1):
    """The offspring of generation 0 and so the plan of its first stage follow from the seed alone (host arithmetic, no
    fitness): the first seed with which that stage is worth a capture -- under ranks, for the share of EVERY rank.  With 4
    blocks and a handful of offspring most stages are not; without a reused stage a comparison of reuse on against off would
    compare nothing."""
    from gptq_gguf_toolkit_amd.suffix_forward import assign_candidates, plan_stage, stage_costs
    for seed in range(400):
        parent = store.flatten(S.initial_parent(ctx, 4.0))
        offs = [store.flatten(o) for o in S.make_offspring(S.initial_parent(ctx, 4.0), offspring, random.Random(seed), ctx, "size")]
        owner = assign_candidates(stage_costs(offs, parent, N_BLOCKS), world_size)
        if all(plan_stage([o for o, r in zip(offs, owner) if r == k], parent, N_BLOCKS, stride)[0] for k in range(world_size)):
            return seed
    raise AssertionError("no seed below 400 gives a first stage that reuses")


def bound(got, a, b, what):
    """got equals a, or lies within the spread of the two plain runs a and b."""
    if torch.is_tensor(got):
        spread, diff = float((a.float() - b.float()).abs().max()), float((got.float() - a.float()).abs().max())
    else:
        spread, diff = abs(a - b), abs(got - a)
    if spread > 0 or diff > 0:
        print(f"{what}: differs by {diff!r}, two plain runs by {spread!r}")
    assert diff <= spread, (what, diff, spread)
    return spread


# ------------------------------------------------------------------------------------------------ 1: suffix equals full
@pytest.mark.parametrize("resident", ["dense", "packed"])
def test_suffix_equals_full(world, resident):
    from gptq_gguf_toolkit_amd.suffix_forward import SuffixRunner
    S, model, store, ctx = searched(world, resident)
    names = world["names"]
    store.switch({n: float((2, 4, 6)[(3 * i + 1) % 3]) for i, n in enumerate(names)})
    data = [world["calib"][0], world["calib"][1][:, :37]]  # the cut last sequence of a minibatch has an odd length
    with torch.no_grad():
        full = [(model(ids.cuda()).logits, model(ids.cuda()).logits) for ids in data]
    spreads = []
    es = 2
    for budget, stride in ((None, 1), (3 * 101 * 256 * es, 2)):
        runner = SuffixRunner(model, budget_bytes=budget)
        runner.capture(data)
        assert runner.stride == stride and sorted(runner._seqs[0].hidden) == ([0, 1, 2, 3, 4] if stride == 1 else [0, 2, 4])
        for i, ids in enumerate(data):
            for b in range(N_BLOCKS + 1):  # with stride 2, start blocks 1 and 3 are no cached boundary
                got = runner.logits(i, b, ids.cuda())
                assert got.dtype == full[i][0].dtype and got.shape == full[i][0].shape
                spreads.append(bound(got, *full[i], f"{world['dtype']} {resident} stride {stride} seq {i} from block {b}"))
    print(f"spread of two full forwards, max over all cases: {max(spreads)!r}")


# ------------------------------------------------------------------------------------------------ 2: reuse happens
@pytest.mark.parametrize("resident", ["dense", "packed"])
@pytest.mark.parametrize("fitness_fn", ["kl", "ppl", "sparse_kl"])
def test_blocks_before_the_change_are_not_run(world, resident, fitness_fn):
    from gptq_gguf_toolkit_amd.suffix_forward import SuffixRunner, first_changed_block
    S, model, store, ctx = searched(world, resident)
    parent = {n: 4.0 for n in world["names"]}
    ids = [0, 3, 5]
    data = [world["calib"][i] for i in ids[:2]] + [world["calib"][ids[2]][:, :37]]
    tg = None
    if fitness_fn == "kl":
        tg = [world["kl"][i] for i in ids[:2]] + [world["kl"][ids[2]][:, :37]]
    elif fitness_fn == "sparse_kl":
        tg = [world["sparse_kl"][i] for i in ids[:2]] + [tuple(t[:, :37] for t in world["sparse_kl"][ids[2]])]
    runner = SuffixRunner(model)
    evaluate = S.suffix_evaluate(store, runner, model, fitness_fn)
    ran = []
    hooks = [blk.register_forward_hook(lambda m, a, o, b=b: ran.append(b)) for b, blk in enumerate(model.model.layers)]
    for layer, level in (("model.layers.2.mlp.down_proj", 2.0), ("model.layers.2.self_attn.q_proj", 6.0)):
        cand = dict(parent, **{layer: level})
        assert first_changed_block(parent, cand, N_BLOCKS) == 2
        plain = [evaluate(cand, data, tg) for _ in range(2)]
        store.switch(parent)
        runner.capture(data)
        del ran[:]
        got = evaluate(cand, data, tg, 2)
        assert ran == [2, 3] * len(data), ran  # blocks 0 and 1 are the parent's: not run
        bound(got, *plain, f"{world['dtype']} {resident} {fitness_fn} {layer}")
        del ran[:]
        got = evaluate(parent, data, tg, N_BLOCKS)
        assert ran == []  # the parent competing in the last stage: the post-block modules only
        bound(got, evaluate(parent, data, tg), evaluate(parent, data, tg), f"{fitness_fn}, the parent itself")
    for h in hooks:
        h.remove()


# ------------------------------------------------------------------------------------------------ 3: stale cache
SEARCH = dict(generations=3, offspring=6, target_bitwidth=4.0, survivors_per_selection=(2, 1), tokens_per_selection=(128, 256),
              group_rule="size", fitness_fn="kl")


def strip(trace):
    """-> (the trace without its fitnesses, the fitnesses in order)."""
    fits = [f for rec in trace for st in rec["stages"] for f in st["fitnesses"]]
    bare = [dict(rec, stages=[{k: v for k, v in st.items() if k != "fitnesses"} for st in rec["stages"]]) for rec in trace]
    return bare, fits


@pytest.mark.parametrize("resident", ["dense", "packed"])
def test_search_with_reuse_is_the_search_without(world, resident):
    from gptq_gguf_toolkit_amd.suffix_forward import StageReuse, SuffixRunner

    S, _, store, ctx = searched(world, resident)
    seed = seed_whose_first_stage_reuses(S, ctx, store, SEARCH["offspring"], stride=2)
    del store

    def run(reuse_bytes):
        S, model, store, ctx = searched(world, resident)
        reuse = runner = None
        if reuse_bytes != "off":
            runner = SuffixRunner(model, budget_bytes=reuse_bytes, log=lambda *a: None)
            reuse = StageReuse(runner, store)
        evaluate = S.suffix_evaluate(store, runner, model, "kl")
        out = S.search(ctx, evaluate, world["calib"], random.Random(seed), target_logits=world["kl"], reuse=reuse, **SEARCH)
        return out, reuse

    (p0, f0, t0), _ = run("off")
    (p1, f1, t1), _ = run("off")
    (pa, fa, ta), ra = run(None)
    # 3 boundaries of 128 tokens: the 128-token stages fit at stride 2 only, the 256-token ones not at all (2 x 256 tokens)
    (pb, fb, tb), rb = run(3 * 128 * 256 * 2)
    # 3 boundaries of 256 tokens: the 128-token stages at stride 1, the 256-token ones -- the parent among them -- at stride 2
    (pc, fc, tc), rc = run(3 * 256 * 256 * 2)
    bare0, fits0 = strip(t0)
    fits1 = strip(t1)[1]
    assert strip(t1)[0] == bare0 and p1 == p0
    spread = max(abs(a - b) for a, b in zip(fits0, fits1))
    print(f"{world['dtype']} {resident}, seed {seed}: {len(fits0)} fitnesses, two plain searches differ by at most {spread!r}")
    for tag, (p, f, t, r) in (("stride 1", (pa, fa, ta, ra)), ("forced stride 2 / no room", (pb, fb, tb, rb)),
                              ("forced stride 1 / 2", (pc, fc, tc, rc))):
        bare, fits = strip(t)
        assert bare == bare0 and p == p0, tag                      # candidates, minibatches, survivors: identical
        worst = max(abs(a - b) for a, b in zip(fits, fits0))
        print(f"  reuse, {tag}: fitnesses differ from the plain search's by at most {worst!r}; "
              f"{sum(st[0] for st in r.stages)} of {len(r.stages)} stages reused, {r.runner.captures} captures")
        assert all(abs(a - b) <= abs(c - b) for a, b, c in zip(fits, fits0, fits1)), tag
        bound(f, f0, f1, tag)
        assert len(r.stages) == 6 and any(st[0] for st in r.stages), r.stages  # a reused stage: the cache was live, then dropped
        assert not r.runner.valid
    assert ra.runner.strides_used == [1] * 6 and rb.runner.strides_used == [2, None] * 3 and rc.runner.strides_used == [1, 2] * 3
    assert ra.stages[0][0] and rb.stages[0][0] and not any(st[0] for st in rb.stages[1::2])


@pytest.mark.parametrize("resident", ["dense", "packed"])
def test_last_stage_over_a_strided_cache(world, resident):
    """One selection as a generation's last stage has it -- the parent among the candidates (it starts after the last block),
    256 tokens (the last sequence cut), the cache forced to stride 2, candidates first changed in blocks 1, 2 and 3 --
    against the same selection without reuse."""
    from gptq_gguf_toolkit_amd.suffix_forward import StageReuse, SuffixRunner
    S, model, store, ctx = searched(world, resident)
    flat_parent = {n: 4.0 for n in world["names"]}
    nested = lambda flat: [[flat[n] for n in g] for g in ctx.names]  # noqa: E731
    parent = nested(flat_parent)
    cands = [nested(dict(flat_parent, **{f"model.layers.{b}.mlp.up_proj": 2.0, "model.layers.3.mlp.gate_proj": 6.0}))
             for b in (3, 1, 2)] + [parent]
    calib = world["calib"][:3] + [c[:, :50] for c in world["calib"][3:]]  # 64- and 50-token sequences: five or six make 256 tokens, the last one cut
    targets = world["kl"][:3] + [t[:, :50] for t in world["kl"][3:]]
    runner = SuffixRunner(model, budget_bytes=3 * 256 * 256 * 2, log=lambda *a: None)
    reuse = StageReuse(runner, store)
    evaluate = S.suffix_evaluate(store, runner, model, "kl")
    plain_traces = [[], []]
    plain = [S.selection(evaluate, cands, 1, calib, 256, random.Random(3), "kl", targets, tr) for tr in plain_traces]
    trace = []
    ran = []
    hooks = [blk.register_forward_hook(lambda m, a, o, b=b: ran.append(b)) for b, blk in enumerate(model.model.layers)]
    got = S.selection(evaluate, cands, 1, calib, 256, random.Random(3), "kl", targets, trace, parent=parent, reuse=reuse)
    for h in hooks:
        h.remove()
    assert reuse.stages == [(True, 2, [2, 0, 2, 4])] and runner.strides_used == [2] and not runner.valid
    n_seq = len(trace[0]["minibatch_ids"])
    # three full forwards of the once-per-model use_cache check, the capture, then candidates from blocks 2, 0, 2 and the parent
    # from no block at all
    assert n_seq >= 5 and ran == list(range(4)) * (3 + n_seq) + [2, 3] * n_seq + list(range(4)) * n_seq + [2, 3] * n_seq, ran
    assert got[0] == plain[0][0] and trace[0]["survivor_ids"] == plain_traces[0][0]["survivor_ids"]
    fits = [tr[0]["fitnesses"] for tr in [trace] + plain_traces]
    assert len(fits[0]) == 4
    for a, b, c in zip(*fits):  # every candidate's fitness, the parent's among them
        bound(a, b, c, f"{world['dtype']} {resident} last stage at stride 2")


# ------------------------------------------------------------------------------------------------ 4: ranks
@pytest.mark.parametrize("reuse", ["on", "off"])
def test_two_ranks_write_the_single_process_result(reuse, tmp_path, tmp_path_factory):
    """python -m torch.distributed.run --nproc-per-node 2 -m gptq_gguf_toolkit_amd.evo_quant_search ... as a fresh child
    (RCCL with two GPUs, else two gloo ranks sharing the one): its configuration file and trace are the single-process run's
    of the same command line."""
    import shutil
    from gptq_gguf_toolkit_amd import evo_quant_search as S
    world = make_world("float16", tmp_path_factory)
    calib = str(world["tmp"] / "calib.pt")
    _, _, store, ctx = searched(world, "dense")
    seed = seed_whose_first_stage_reuses(S, ctx, store, 12, stride=1, world_size=2)  # each rank plans for its own share
    del store

    def argv(db, trace):
        return ["--model_name_or_path", str(world["tmp"] / "hf"), "--dtype", "float16", "--calibration_data", calib,
                "--eval_datasets", calib, "--calibration_tokens", "512", "--eval_tokens", "192",
                "--calibration_sequence_length", "64", "--eval_sequence_length", "64", "--generations", "2", "--offspring", "12",
                "--target_bitwidth", "4", "--quant_weights_path", str(db), "--survivors_per_selection", "3", "1",
                "--tokens_per_selection", "128", "256", "--reuse_prefix", reuse, "--trace_out", str(trace), "--seed", str(seed)]

    one, two = tmp_path / "one", tmp_path / "two"
    shutil.copytree(world["db"], one)
    shutil.copytree(world["db"], two)
    parent, out1 = S.main(argv(one, tmp_path / "one.json"))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    backend = [] if torch.cuda.device_count() >= 2 else ["--backend", "gloo"]
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(23000 + os.getpid() % 2000), "-m",
           "gptq_gguf_toolkit_amd.evo_quant_search"] + argv(two, tmp_path / "two.json") + backend
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    name = S.configuration_name("kl", 4.0)
    written = sorted(f for f in os.listdir(two) if f.startswith("evo-"))
    assert written == [name] and not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]  # exactly one file, no leftovers
    assert open(two / name).read() == open(out1).read()
    t1, t2 = json.load(open(tmp_path / "one.json")), json.load(open(tmp_path / "two.json"))
    worst = max(abs(a - b) for a, b in zip(strip(t1)[1], strip(t2)[1]))
    print(f"reuse {reuse}: fitnesses of the two-rank run differ from the single process's by at most {worst!r}")
    assert strip(t2)[0] == strip(t1)[0]
    assert t2 == t1
    assert p.stdout.count("Final configuration:") == 1  # rank 0 alone prints
    m = re.search(r"reuse_prefix: (\d+) of (\d+) stages", p.stdout)
    assert (m is not None and int(m.group(1)) > 0 and int(m.group(2)) == 4) if reuse == "on" else m is None
