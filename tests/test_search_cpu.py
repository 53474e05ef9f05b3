"""Bit-width search, host side (no GPU): the gq_level_switch symbol and its argument checks, the search's host logic
(evo_quant_search.py) on a fake model (modules with weight.numel() only) and a fitness that is a fixed function of the
state, the reference's own trajectory (fixture G19, tests/golden/make_golden_search.py), the configuration file's format
and ppleval.load_compressed_weights on the search's configuration lines."""
import ctypes
import os
import random
import re
import types

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden

torch = pytest.importorskip("torch")


# ------------------------------------------------------------------------------------------------ the C ABI
def test_level_switch_symbol_is_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_search.h")).read()
    declared = set(re.findall(r"\b(gq_[a-z0-9_]+)\s*\(", hdr))
    L = _cabi.lib()
    assert declared == set(_cabi.EXPORTS_SEARCH) == {"gq_level_switch"}
    assert not declared & set(_cabi.EXPORTS) and not declared & set(_cabi.EXPORTS_ERREST)
    assert len(_cabi.EXPORTS) == 48 and set(_cabi.EXPORTS_ERREST) == {"gq_quad_form", "gq_quad_form_workspace_bytes"}
    for sym in declared:
        assert hasattr(ctypes.CDLL(_cabi.SO_PATH), sym) and hasattr(L, sym), sym
        assert getattr(L, sym).argtypes, f"{sym} has no argtypes"
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6  # additive: the version stays
    m = re.search(r"#define GQ_SWITCH_MAX_JOBS (\d+)", hdr)
    assert m and int(m.group(1)) == _cabi.SWITCH_MAX_JOBS
    # the C struct and its ctypes image: 3 pointers, 2 int64, 2 int32
    assert ctypes.sizeof(_cabi.SwitchJob) == 48 and _cabi.SwitchJob.kind.offset == 40 and _cabi.SwitchJob.out_dtype.offset == 44
    assert "evopress/evo_quant_search.py:110-138" in hdr
    assert "`gq_level_switch`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_level_switch_argument_checks_need_no_device():
    """Every refusal comes before the first HIP call: a negative status and a message naming the job and the argument."""
    from gptq_gguf_toolkit_amd import _cabi
    L, J = _cabi.lib(), _cabi.SwitchJob
    p = 256  # any 16-byte aligned address, never dereferenced

    def refused(jobs, status, *words):
        arr = (J * len(jobs))(*jobs)
        rc = L.gq_level_switch(arr, len(jobs), None)
        msg = L.gq_last_error().decode()
        assert rc == status and all(w in msg for w in words), (rc, msg)

    ok = J(p, p, None, 4, 256, 12, 1)
    assert L.gq_level_switch(None, 0, None) == 0                      # n_jobs = 0: a no-op, the table is not read
    assert L.gq_level_switch((J * 1)(ok), 0, None) == 0
    assert L.gq_level_switch((J * 1)(ok), -1, None) == -2 and "n_jobs" in L.gq_last_error().decode()
    assert L.gq_level_switch(None, 1, None) == -6 and "jobs_host" in L.gq_last_error().decode()
    refused([J(None, p, None, 4, 256, 12, 1)], -6, "job 0", "src is NULL")
    refused([ok, J(p, None, None, 4, 256, 12, 1)], -6, "job 1", "dst is NULL")
    refused([ok, ok, J(p, p, None, 4, 256, 9, 1)], -1, "job 2", "kind 9")
    refused([J(p, p, None, 4, 256, 15, 1)], -1, "job 0", "kind 15")
    refused([J(p, p, None, 4, 256, 3, 1)], -1, "job 0", "kind 3")
    refused([J(p, p, None, 4, 256, 12, 3)], -1, "job 0", "out_dtype 3")
    refused([J(p, p, None, 4, 384, 12, 1)], -2, "job 0", "C=384")   # packed: C % 256
    refused([J(p, p, None, 0, 256, 12, 1)], -2, "job 0", "R=0")
    refused([J(p, p, None, -3, 256, 1, 1)], -2, "job 0", "R=-3")
    refused([J(p, p, None, 4, 0, 1, 1)], -2, "job 0", "C=0")
    refused([J(p, p + 8, None, 4, 256, 12, 1)], -2, "job 0", "dst not 16-byte aligned")
    refused([J(p + 8, p, None, 4, 256, 12, 1)], -2, "job 0", "src not 16-byte aligned")   # Q4_K: 16
    refused([J(p + 8, p, None, 4, 256, 13, 1)], -2, "job 0", "src not 16-byte aligned")   # Q5_K: 16
    refused([J(p + 2, p, None, 4, 256, 10, 1)], -2, "job 0", "src not 4-byte aligned")    # Q2_K: 4
    refused([J(p + 1, p, None, 4, 256, 11, 1)], -2, "job 0", "src not 2-byte aligned")    # Q3_K: 2
    refused([J(p + 3, p, None, 4, 256, 14, 1)], -2, "job 0", "src not 2-byte aligned")    # Q6_K: 2
    refused([J(p, p, 258, 4, 256, 12, 1)], -2, "job 0", "row_src")
    refused([J(p + 4, p, None, 4, 256, 1, 2)], -2, "job 0", "src not 16-byte aligned")    # dense
    refused([J(p, p, None, 4, 260, 1, 2)], -2, "job 0", "C=260")     # fp16 rows of 520 bytes
    refused([J(p, p, None, 4, 252, 0, 1)], -2, "job 0", "C=252")     # fp32 rows fit, fp16 rows of 504 bytes do not
    refused([J(p, p, None, 1 << 50, 256, 12, 1)], -2, "job 0", "more than one launch")
    # the refusal of a late job comes before any launch of the earlier ones: 70 jobs, the last one bad
    refused([ok] * 69 + [J(p, None, None, 4, 256, 12, 1)], -6, "job 69", "dst is NULL")


def test_ops_level_switch_refuses_cpu_tensors_and_takes_an_empty_list():
    from gptq_gguf_toolkit_amd import _cabi, ops
    assert ops.level_switch([]) is None
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.level_switch([(torch.zeros(4, 256), torch.zeros(4, 256, dtype=torch.float16), None, None)])


# ------------------------------------------------------------------------------------------------ the fake search problem
BWS = [(2.5625, "2.5625-Q2_K.pth"), (3.4375, "3.4375-Q3_K.pth"), (4.5, "4.5-Q4_K.pth"), (5.5, "5.5-Q5_K.pth"),
       (6.5625, "6.5625-Q6_K.pth")]
BWS4 = sorted(BWS + [(4.0, "4-Q4_0.pth")])  # with a level at the integer target: the first parent is within budget
NUMEL = {"self_attn.q_proj": 65536, "self_attn.k_proj": 16384, "self_attn.v_proj": 16384, "self_attn.o_proj": 65536,
         "mlp.gate_proj": 131072, "mlp.up_proj": 131072, "mlp.down_proj": 131072}


class FakeModel:
    """modules with weight.numel() only"""

    def __init__(self, blocks=3):
        self.numel = {f"model.layers.{b}.{k}": n for b in range(blocks) for k, n in NUMEL.items()}

    def get_submodule(self, name):
        n = self.numel[name]
        return types.SimpleNamespace(weight=types.SimpleNamespace(numel=lambda: n))


def problem(group_rule, target, blocks=3, bws=BWS4):
    from gptq_gguf_toolkit_amd import evo_quant_search as S
    model = FakeModel(blocks)
    names = sorted(model.numel, key=S.layer_order_fn)
    levels = {n: list(bws) for n in names}
    grouped = S.group_layers(model, names, group_rule)
    return S, S._Ctx(model, grouped, levels, S.target_bits_of(grouped, model, target)), model


def fake_fitness(ctx):
    """A fixed function of the state: every layer's numel x 2^-bitwidth, weighted by its position."""
    w = {n: 1.0 + 0.37 * ((7 * i) % 5) for i, n in enumerate(n for g in ctx.names for n in g)}

    def evaluate(candidate, data, targets):
        return sum(w[n] * ctx.model.get_submodule(n).weight.numel() * 2.0 ** (-bw)
                   for names, bws in zip(ctx.names, candidate) for n, bw in zip(names, bws))
    return evaluate


CALIB = [torch.zeros(1, 64, dtype=torch.long) for _ in range(12)]


def run(group_rule, target, seed, generations=6, **kw):
    S, ctx, _ = problem(group_rule, target)
    args = dict(generations=generations, offspring=8, target_bitwidth=target, survivors_per_selection=(3, 1),
                tokens_per_selection=(100, 200), group_rule=group_rule, fitness_fn="ppl")
    args.update(kw)
    return (S, ctx) + S.search(ctx, fake_fitness(ctx), CALIB, random.Random(seed), **args)


@pytest.mark.parametrize("group_rule,target", [("size", 4.0), ("name", 4.0), ("none", 4.0), ("size", 3.7), ("none", 3.7)])
def test_search_invariants(group_rule, target):
    extra = dict(initially_generated=5, initial_tokens=128) if target != int(target) else {}
    S, ctx, parent, fit, trace = run(group_rule, target, seed=3, **extra)
    index = {bw: i for i, (bw, _) in enumerate(BWS4)}
    gens = [r for r in trace if "parent" in r]
    assert len(gens) == 6
    if extra:
        init = trace[0]["initial"]
        assert len(init["candidates"]) == 5 and init["num_tokens"] == 128
        assert all(ctx.bits(c) <= ctx.target_bits for c in init["candidates"])
    for rec in gens:
        par, offs = rec["parent"], rec["offspring"]
        assert ctx.bits(par) <= ctx.target_bits and all(ctx.bits(o) <= ctx.target_bits for o in offs)
        # no duplicate, no copy of the parent
        assert all(o != par for o in offs) and all(a != b for i, a in enumerate(offs) for b in offs[:i])
        assert 1 <= len(offs) <= 8
        if group_rule != "none":
            for o in offs:  # a flip lowers one layer and raises one layer OF THE SAME GROUP by one level each
                for g_par, g_off in zip(par, o):
                    steps = [index[b] - index[a] for a, b in zip(g_par, g_off)]
                    assert sum(steps) <= 0 and (not any(s > 0 for s in steps) or any(s < 0 for s in steps))
        # the parent joins exactly the last selection stage
        first, last = rec["stages"]
        assert first["candidates"] == offs and par not in first["candidates"] and first["num_tokens"] == 100
        assert last["candidates"][-1] == par and last["candidates"].count(par) == 1 and last["num_tokens"] == 200
        assert last["candidates"][:-1] == [first["candidates"][i] for i in first["survivor_ids"]]
        assert len(first["survivor_ids"]) == min(3, len(offs)) and len(last["survivor_ids"]) == 1
        # elitism
        assert min(last["fitnesses"]) == last["fitnesses"][last["survivor_ids"][0]] <= last["fitnesses"][-1]
    assert ctx.bits(parent) <= ctx.target_bits
    assert fit == fake_fitness(ctx)(parent, None, None)
    fits = [fake_fitness(ctx)(r["parent"], None, None) for r in gens] + [fit]
    assert all(b <= a for a, b in zip(fits, fits[1:]))  # elitism across generations: the fitness ignores the minibatch


def test_same_seed_same_trajectory_and_another_seed_another():
    a, b, c = (run("size", 4.0, seed=s)[2:] for s in (11, 11, 12))
    assert a == b
    assert a[2] != c[2]


def test_minibatch_holds_exactly_num_tokens_from_distinct_sequences():
    from gptq_gguf_toolkit_amd import evo_quant_search as S
    data = [torch.full((1, L), i) for i, L in enumerate([64, 48, 64, 100, 64, 31, 64])]
    targets = [torch.full((1, d.shape[1], 4), float(i)) for i, d in enumerate(data)]
    sparse = [(t[..., :2], t[..., :2].long()) for t in targets]
    for seed in range(20):
        for num_tokens in (1, 64, 150, 300):
            mb, ids, tg = S.minibatch(data, num_tokens, random.Random(seed), "kl", targets)
            assert sum(x.shape[1] for x in mb) == num_tokens and len(set(ids)) == len(ids) == len(mb) == len(tg)
            for x, i, t in zip(mb, ids, tg):
                assert bool((x == i).all()) and t.shape[:2] == x.shape and bool((t == i).all())
            assert all(x.shape[1] == data[i].shape[1] for x, i in zip(mb[:-1], ids[:-1]))  # only the last one is cut
            mb2, ids2, tg2 = S.minibatch(data, num_tokens, random.Random(seed), "sparse_kl", sparse)
            assert ids2 == ids and all(v.shape[:2] == x.shape == k.shape[:2] for x, (v, k) in zip(mb2, tg2))
            assert S.minibatch(data, num_tokens, random.Random(seed), "ppl")[1:] == (ids, None)


def test_budget_helpers():
    S, ctx, model = problem("size", 4.0, blocks=1, bws=BWS)
    state = S.initial_parent(ctx, 4.0)
    assert state == [[4.5, 4.5, 4.5], [4.5, 4.5], [4.5, 4.5]]  # down gate up | k v | o q: 4 is no level, 4.5 the closest
    assert ctx.bits(state) == 4.5 * sum(NUMEL.values()) > ctx.target_bits == 4 * sum(NUMEL.values())
    assert ctx.next_bw(state, 0, 0, "decrease") == 3.4375 and ctx.next_bw(state, 0, 0, "increase") is None
    low = [[2.5625, 2.5625, 2.5625], [2.5625, 2.5625], [2.5625, 2.5625]]
    assert ctx.next_bw(low, 2, 1, "decrease") is None and ctx.next_bw(low, 2, 1, "increase") == 3.4375
    top = [[6.5625] * len(g) for g in ctx.names]
    assert ctx.next_bw(top, 1, 0, "increase") is None
    assert S.initial_parent(ctx, 6.0) == [[5.5] * len(g) for g in ctx.names]
    assert S.initial_parent(ctx, 3.0) == [[2.5625] * len(g) for g in ctx.names]  # a tie goes to the lower level (min's first)
    assert S.target_bits_of(ctx.names, model, 3.7) == sum(int(n * 3.7) for n in NUMEL.values())
    # an over-budget parent (the integer target is no level): every offspring is brought under the budget first
    for rule in ("size", "none"):
        S, ctx, _ = problem(rule, 4.0, bws=BWS)
        par = S.initial_parent(ctx, 4.0)
        offs = S.make_offspring(par, 6, random.Random(5), ctx, rule)
        assert len(offs) == 6 and all(ctx.bits(o) <= ctx.target_bits < ctx.bits(par) for o in offs)


def test_scan_available_bitwidths_reads_both_layouts(tmp_path):
    from gptq_gguf_toolkit_amd import evo_quant_search as S
    hf = tmp_path / "hf" / "model.layers.0.mlp.up_proj"
    hf.mkdir(parents=True)
    for f in ("6.5625-Q6_K.pth", "2.5625-Q2_K.pth", "4.5-Q4_K.pth"):
        (hf / f).write_bytes(b"")
    (hf / "4.5-Q4_K-metadata.json").write_text("{}")
    (tmp_path / "hf" / "manifest.json").write_text("{}")
    assert S.scan_available_bitwidths(str(tmp_path / "hf")) == {
        "model.layers.0.mlp.up_proj": [(2.5625, "2.5625-Q2_K.pth"), (4.5, "4.5-Q4_K.pth"), (6.5625, "6.5625-Q6_K.pth")]}
    gg = tmp_path / "gg" / "blk.0.ffn_up.weight"
    gg.mkdir(parents=True)
    for f in ("4.pth", "2.pth"):
        (gg / f).write_bytes(b"")
    assert S.scan_available_bitwidths(str(tmp_path / "gg"), ["model.layers.0.mlp.up_proj"]) == {
        "model.layers.0.mlp.up_proj": [(2.0, "2.pth"), (4.0, "4.pth")]}


def test_configuration_file_format_byte_for_byte():
    from gptq_gguf_toolkit_amd import evo_quant_search as S
    grouped = (["model.layers.0.self_attn.q_proj", "model.layers.1.self_attn.q_proj"], ["model.layers.0.mlp.up_proj"])
    levels = {n: list(BWS) for g in grouped for n in g}
    levels["model.layers.0.mlp.up_proj"] = [(4.0, "4-Q4_K.pth"), (6.0, "6-Q6_K.pth")]
    text = S.configuration_text(grouped, [[4.5, 2.5625], [6.0]], levels)
    assert text == ("model.layers.0.self_attn.q_proj: 4.5 (4.5-Q4_K.pth)\n"
                    "model.layers.1.self_attn.q_proj: 2.5625 (2.5625-Q2_K.pth)\n"
                    "model.layers.0.mlp.up_proj: 6.0 (6-Q6_K.pth)")
    assert S.configuration_name("kl", 3.7) == "evo-kl-configuration-3.7.txt"
    assert S.configuration_name("ppl", 4.0) == "evo-ppl-configuration-4.0.txt"


# ------------------------------------------------------------------------------------------------ the reference's trajectory
@pytest.mark.parametrize("group_rule", ["size", "name", "none"])
def test_reference_trajectory_golden(group_rule):
    """G19: the reference's main() driven with a stub model, stub data and the fixed fitness below, one seed per group
    rule; every candidate it evaluated, in order, and its final configuration text -- and the same from this package."""
    import sys
    sys.path.insert(0, GOLDEN)
    import make_golden_search as M
    g = load_golden("G19_search")
    got_states, got_text = M.ours(group_rule)
    assert np.array_equal(np.asarray(got_states, dtype=np.float64), g[f"{group_rule}_states"])
    assert got_text == bytes(g[f"{group_rule}_config"]).decode()


# ------------------------------------------------------------------------------------------------ ppleval reads the result
def test_load_compressed_weights_reads_search_and_plain_configurations(tmp_path):
    from gptq_gguf_toolkit_amd import ppleval
    names = ["layers.0.a", "layers.0.b"]

    def model():
        m = torch.nn.Module()
        m.layers = torch.nn.ModuleList([torch.nn.Module()])
        m.layers[0].a, m.layers[0].b = torch.nn.Linear(8, 4, bias=False), torch.nn.Linear(8, 4, bias=False)
        return m.half()

    g = torch.Generator().manual_seed(0)
    w = {}
    for n in names:
        (tmp_path / n).mkdir()
        for f in ("4-Q4_K.pth", "4.5-Q4_K.pth", "4.5-Q5_K.pth", "3.pth"):
            w[n, f] = torch.randn(4, 8, generator=g)
            torch.save(w[n, f], tmp_path / n / f)
    cfg = tmp_path / "evo-kl-configuration-4.0.txt"
    cfg.write_text("layers.0.a: 4.5 (4.5-Q5_K.pth)\nlayers.0.b: 4.0 (4-Q4_K.pth)")  # the search's lines: the file is named
    m = ppleval.load_compressed_weights(model(), str(tmp_path), str(cfg))
    assert torch.equal(m.layers[0].a.weight, w["layers.0.a", "4.5-Q5_K.pth"].half())  # "4.5" alone names two files
    assert torch.equal(m.layers[0].b.weight, w["layers.0.b", "4-Q4_K.pth"].half())
    plain = tmp_path / "plain.txt"
    plain.write_text("layers.0.a: 3\nlayers.0.b: 4-Q4_K\n")                          # lines that worked before: the same files
    m = ppleval.load_compressed_weights(model(), str(tmp_path), str(plain))
    assert torch.equal(m.layers[0].a.weight, w["layers.0.a", "3.pth"].half())
    assert torch.equal(m.layers[0].b.weight, w["layers.0.b", "4-Q4_K.pth"].half())
    amb = tmp_path / "amb.txt"
    amb.write_text("layers.0.a: 4.5")  # without the file name "4.5" names two files, as before
    with pytest.raises(FileNotFoundError, match="4.5-Q4_K"):
        ppleval.load_compressed_weights(model(), str(tmp_path), str(amb))
    with pytest.raises(FileNotFoundError, match="9-Q9_K.pth"):
        bad = tmp_path / "bad.txt"
        bad.write_text("layers.0.a: 9.0 (9-Q9_K.pth)")
        ppleval.load_compressed_weights(model(), str(tmp_path), str(bad))


def test_cli_refuses_before_any_work(tmp_path, capsys):
    from gptq_gguf_toolkit_amd import evo_quant_search as S
    ids = tmp_path / "ids.pt"
    torch.save([torch.zeros(1, 8, dtype=torch.long)], ids)
    base = ["--model_name_or_path", "none", "--quant_weights_path", str(tmp_path), "--generations", "1", "--offspring", "2",
            "--target_bitwidth", "4", "--survivors_per_selection", "2", "1", "--tokens_per_selection", "8", "16"]
    ok = S.parse_args(base + ["--calibration_data", str(ids), "--eval_datasets", str(ids)])
    assert (ok.group_rule, ok.fitness_fn, ok.kl_topk, ok.eval_every, ok.dtype, ok.seed, ok.targets_on, ok.calibration_tokens) == \
        ("size", "kl", 10, 1, "auto", 0, "device", 524288)
    for extra, word in ((["--calibration_data", "fineweb_edu", "--eval_datasets", str(ids)], "calibration_data must be a .pt file"),
                        (["--calibration_data", str(ids)], "eval_datasets must be a .pt file"),  # the reference's default names
                        (["--calibration_data", str(ids), "--eval_datasets", str(ids), "--target_bitwidth", "3.5"], "initially_generated"),
                        (["--calibration_data", str(ids), "--eval_datasets", str(ids), "--survivors_per_selection", "2", "2"], "one survivor"),
                        (["--calibration_data", str(ids), "--eval_datasets", str(ids), "--tokens_per_selection", "8"], "same number of stages")):
        with pytest.raises(SystemExit):
            S.parse_args(base + extra)
        assert word in capsys.readouterr().err
    try:
        import wandb  # noqa: F401
    except ModuleNotFoundError:
        with pytest.raises(SystemExit):
            S.parse_args(base + ["--calibration_data", str(ids), "--eval_datasets", str(ids), "--log_wandb"])
        assert "wandb" in capsys.readouterr().err


def test_level_store_host_logic_on_a_stand_in_switch(tmp_path, monkeypatch):
    """LevelStore's scan, diff and bookkeeping with ops.level_switch replaced by a torch copy (dense levels, CPU tensors): one
    call per switch over exactly the changed Linears, weights written in place, the nested-list form of a state."""
    from gptq_gguf_toolkit_amd import level_store as LS
    m = torch.nn.Module()
    m.layers = torch.nn.ModuleList([torch.nn.Module()])
    m.layers[0].a, m.layers[0].b = torch.nn.Linear(8, 4, bias=False), torch.nn.Linear(8, 4, bias=False)
    m.half()
    names, g, w = ["layers.0.a", "layers.0.b"], torch.Generator().manual_seed(1), {}
    for n in names:
        (tmp_path / n).mkdir()
        for f in ("2-Q2_K.pth", "4-Q4_K.pth"):
            w[n, f] = torch.randn(4, 8, generator=g)
            torch.save(w[n, f], tmp_path / n / f)
    calls = []

    def fake_switch(jobs):
        calls.append(len(jobs))
        for src, dst, kind, rows in jobs:
            assert kind is None and rows is None
            dst.copy_(src.to(dst.dtype))

    monkeypatch.setattr(LS.ops, "level_switch", fake_switch)
    store = LS.LevelStore(m, str(tmp_path), "cpu")
    assert list(store.layers) == names and store.level_keys("layers.0.a") == [2.0, 4.0]
    assert store.bytes() == 4 * 4 * 8 * 4  # four fp32 levels, kept in the dtype they were saved in
    ptrs = [m.get_submodule(n).weight.data_ptr() for n in names]
    assert store.switch({n: 4.0 for n in names}) == 2
    assert store.switch({"layers.0.a": 2.0, "layers.0.b": 4.0}) == 1
    store.grouped_layer_names = [["layers.0.b"], ["layers.0.a"]]
    assert store.switch([[4.0], [2.0]]) == 0 and store.switch([[2.0], [2.0]]) == 1
    assert calls == [2, 1, 0, 1] and store.jobs_issued == 4
    assert torch.equal(m.layers[0].a.weight.data, w["layers.0.a", "2-Q2_K.pth"].half())
    assert torch.equal(m.layers[0].b.weight.data, w["layers.0.b", "2-Q2_K.pth"].half())
    assert [m.get_submodule(n).weight.data_ptr() for n in names] == ptrs
    with pytest.raises(KeyError, match="no level 3.0"):
        store.switch({"layers.0.a": 3.0})
    with pytest.raises(MemoryError, match=r"need \d+ bytes on cpu, 100 are available"):
        LS.LevelStore(m, str(tmp_path), "cpu", capacity_bytes=100)
