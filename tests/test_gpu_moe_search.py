"""-m gpu: K30, the bit-width search on a fused-expert model.  gq_level_switch_experts against gq_level_switch with the E
per-expert jobs (equal bits), LevelStore's expert units on both residencies against gguf_loader's reading of the uniform .gguf
files the database was cut from, and evo_quant_search on the tiny Mixtral of tests/moe_gguf.py: the trace repeats, with and
without --reuse_prefix, and the stitched .gguf scores what the search reported."""
import io
import json
import os
import sys
from contextlib import redirect_stdout

import pytest

import moe_gguf
import moe_level_db as MDB
from conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
PACKED_KINDS = {"Q2_K": 10, "Q3_K": 11, "Q4_K": 12, "Q5_K": 13, "Q6_K": 14, "Q8_0": 8, "IQ4_NL": 20, "IQ4_XS": 23}
DENSE_KINDS = {"F32": F32, "F16": F16, "BF16": BF16}
SHAPES = ((1, 256), (7, 768), (64, 512))  # (7, 768): 21 blocks per expert -- a partial last unit, expert boundaries inside a turn
EXPERTS = (1, 3, 5)
GUARD = 64      # bytes before and after every destination buffer
FILL = 0xA5     # the sentinel byte


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from gptq_gguf_toolkit_amd import ops as _ops
    return _ops


def raw(t):
    """Any tensor as its bytes."""
    return t.contiguous().view(torch.uint8)


def source(ops, kind, E, R, C, seed):
    """(src on the device, kind for the bindings, [the E per-expert sources]) of one stacked tensor: uniformly random block bytes,
    or random dense values.  (Random bytes hold NaN / Inf scales in a few blocks: every comparison below is on bits.)"""
    g = torch.Generator().manual_seed(seed)
    if kind in PACKED_KINDS:
        t = PACKED_KINDS[kind]
        bs, ts = ops.block_geometry(t)
        src = torch.randint(0, 256, (E * R * (C // bs) * ts,), dtype=torch.uint8, generator=g).cuda()
        return src, t, [src.view(E, -1)[e] for e in range(E)]
    src = (torch.randn(E, R, C, generator=g) * 3).to(DENSE_KINDS[kind]).cuda()
    return src, None, [src[e] for e in range(E)]


class Dest:
    """A destination buffer of `n` elements with GUARD bytes of sentinel on both sides, all of it pre-filled with the sentinel."""

    def __init__(self, n, dtype):
        es = torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((GUARD + n * es + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.t = self.buf[GUARD:GUARD + n * es].view(dtype)
        assert self.t.data_ptr() % 16 == 0

    def guards_intact(self):
        return bool((self.buf[:GUARD] == FILL).all()) and bool((self.buf[-GUARD:] == FILL).all())


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("kind", list(PACKED_KINDS) + list(DENSE_KINDS))
def test_stacked_job_equals_the_per_expert_jobs(ops, kind):
    """Every (E, shape, out dtype, destination stride): the bits of ops.level_switch over the E per-expert jobs; the half of a
    [E, 2R, C] buffer the job does not name, and the guards around every buffer, keep the sentinel."""
    n = 0
    for E in EXPERTS:
        for R, C in SHAPES:
            src, k, per_expert = source(ops, kind, E, R, C, seed=1000 * E + R)
            for dt in (F32, F16, BF16):
                want = Dest(E * R * C, dt)
                ops.level_switch([(s, want.t.view(E, R, C)[e], k, None) for e, s in enumerate(per_expert)])
                want_bytes = raw(want.t.view(E, R * C))
                assert want.guards_intact()
                # the packed destination [E, R, C]
                got = Dest(E * R * C, dt)
                assert ops.level_switch_experts([(src, got.t.view(E, R, C), k)]) is None
                assert torch.equal(raw(got.t.view(E, R * C)), want_bytes) and got.guards_intact(), (kind, E, R, C, dt, "packed")
                # the gate half and the up half of a fused [E, 2R, C] buffer
                for half in (0, 1):
                    fused = Dest(E * 2 * R * C, dt)
                    view = fused.t.view(E, 2 * R, C)[:, half * R:(half + 1) * R]
                    other = fused.t.view(E, 2 * R, C)[:, (1 - half) * R:(2 - half) * R]
                    ops.level_switch_experts([(src, view, k)])
                    assert torch.equal(raw(view.reshape(E, R * C)), want_bytes), (kind, E, R, C, dt, "half", half)
                    assert bool((raw(other.reshape(E, R * C)) == FILL).all()) and fused.guards_intact(), (kind, E, R, C, dt, half)
                n += 3
    assert n == 81


def test_more_jobs_than_one_launch_takes(ops):
    """GQ_SWITCH_EXPERTS_MAX_JOBS + 1 tiny jobs of mixed kinds in one call (two launches), and the empty call."""
    kinds = list(PACKED_KINDS) + list(DENSE_KINDS)
    n = ops.SWITCH_EXPERTS_MAX_JOBS + 1
    assert n == 72
    jobs, ref, outs, wants = [], [], [], []
    for i in range(n):
        kind, E, (R, C) = kinds[i % len(kinds)], 1 + i % 3, ((1, 256), (2, 512))[i % 2]
        src, k, per_expert = source(ops, kind, E, R, C, seed=i)
        got, want = Dest(E * R * C, F16), Dest(E * R * C, F16)
        jobs.append((src, got.t.view(E, R, C), k))
        ref += [(s, want.t.view(E, R, C)[e], k, None) for e, s in enumerate(per_expert)]
        outs.append(got)
        wants.append(want)
    ops.level_switch(ref)
    ops.level_switch_experts(jobs)
    for i, (got, want) in enumerate(zip(outs, wants)):
        assert torch.equal(got.buf, want.buf), i
    before = [g.buf.clone() for g in outs[:3]]
    assert ops.level_switch_experts([]) is None  # n_jobs == 0: a no-op
    assert all(torch.equal(a, g.buf) for a, g in zip(before, outs))


def test_binding_refuses_views_the_kernel_cannot_fill(ops):
    from gptq_gguf_toolkit_amd._cabi import GQError
    src, k, _ = source(ops, "Q4_K", 2, 4, 256, seed=5)
    dst = torch.zeros(2, 4, 512, dtype=F16, device="cuda")
    with pytest.raises(GQError, match="contiguous"):
        ops.level_switch_experts([(src, dst[:, :, :256], k)])       # rows that are not contiguous
    with pytest.raises(GQError, match="must be 1152 uint8"):
        ops.level_switch_experts([(src[:-144], torch.zeros(2, 4, 256, dtype=F16, device="cuda"), k)])
    with pytest.raises(GQError, match=r"job 0.*dst_expert_stride=1028"):  # 2056 bytes: no multiple of 16
        ops.level_switch_experts([(src, torch.zeros(2, 1028, dtype=F16, device="cuda")[:, :1024].view(2, 4, 256), k)])


# ------------------------------------------------------------------------------------------------ the model and its database
@pytest.fixture(scope="module")
def world(ops, tmp_path_factory):
    """The tiny Mixtral, its six uniform .gguf files and the database cut from them.  The HF directory the tests load is the
    model as the F16 file holds it, so that token_embd / output (Q6_K in every file), the router and the norms are the same
    numbers whether a model comes from that directory or from any of the files."""
    from make_golden_shim import tiny_calib
    from gptq_gguf_toolkit_amd import gguf_loader
    tmp = tmp_path_factory.mktemp("moe_search")
    moe_gguf.build_hf(tmp / "hf0")
    built = MDB.build(moe_gguf.load_hf(tmp / "hf0"), tmp)
    gguf_loader.load_into_model(moe_gguf.load_hf(tmp / "hf0"), built["files"]["F16"]).save_pretrained(
        str(tmp / "hf"), safe_serialization=True)
    ids = tiny_calib(n=8, L=64, seed=31)
    torch.save(ids, str(tmp / "ids.pt"))
    return dict(tmp=tmp, hf=str(tmp / "hf"), db=built["db"], files=built["files"], ids=ids, ids_pt=str(tmp / "ids.pt"))


def i16(t):
    return t.contiguous().view(torch.int16)


def test_database_holds_every_level_of_every_unit(world):
    from gptq_gguf_toolkit_amd import level_db
    for u in MDB.UNITS + MDB.ATTENTION:
        files = level_db.level_files(level_db.layer_dir(world["db"], u))
        assert files == sorted((MDB.level_file(n) for n in MDB.LEVELS), key=level_db.level_key), u
    rec = level_db.read_sidecar(os.path.join(world["db"], "blk.1.ffn_down_exps.weight", "4.25-IQ4_XS.pth"))
    assert rec.shape == (moe_gguf.E, moe_gguf.H, moe_gguf.I) and rec.np_shape == [moe_gguf.E, moe_gguf.H, moe_gguf.I // 256 * 136]
    w = level_db.load_level(rec.path, "cuda", world["db"])
    assert w.dtype == F16 and tuple(w.shape) == rec.shape


def test_dense_store_writes_the_files_tensors_into_the_fused_parameters(world):
    from gptq_gguf_toolkit_amd import gguf_loader
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    model = moe_gguf.load_hf(world["hf"])
    store = LevelStore(model, world["db"], "cuda")  # default discovery: the units, and every Linear the database has (output.weight too)
    assert sorted(store.layers) == sorted(MDB.UNITS + MDB.ATTENTION + ["lm_head"]) and sorted(store.units) == sorted(MDB.UNITS)
    experts = [model.model.layers[n].mlp.experts for n in range(moe_gguf.LAYERS)]
    ptrs = [(ex.gate_up_proj.data_ptr(), ex.down_proj.data_ptr()) for ex in experts]
    issued = 0
    for name in MDB.LEVELS:
        assert store.switch(MDB.uniform_state(name)) == len(MDB.UNITS) + len(MDB.ATTENTION)
        issued += len(MDB.UNITS) + len(MDB.ATTENTION)
        assert store.jobs_issued == issued  # a unit is one job
        want = gguf_loader.load_state_dict(world["files"][name], "cuda", F16)
        have = model.state_dict()
        assert {f"{n}.weight" for n in MDB.ATTENTION} | {f"model.layers.{n}.mlp.experts.{p}" for n in range(moe_gguf.LAYERS)
                                                        for p in ("gate_up_proj", "down_proj")} <= set(want) <= set(have)
        for k, v in want.items():  # every tensor of the file, the searched ones among them
            assert torch.equal(i16(have[k]), i16(v)), (name, k)
        key = MDB.LEVELS[name][1]
        u = MDB.UNITS[4]  # layer 1, up
        assert torch.equal(i16(store.weight_of(u, key)), i16(experts[1].gate_up_proj.data[:, moe_gguf.I:]))
        lt = store.level_tensor(u, key)
        assert lt.dtype == F16 and tuple(lt.shape) == (moe_gguf.E, moe_gguf.I, moe_gguf.H)
    # one unit switched: every other tensor of the model keeps its bits, the parameters their storage
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert store.switch({"model.layers.0.mlp.experts.gate_proj": 2.5625}) == 1 and store.jobs_issued == issued + 1
    q2 = gguf_loader.load_state_dict(world["files"]["Q2_K"], "cuda", F16)
    for k, v in model.state_dict().items():
        if k == "model.layers.0.mlp.experts.gate_up_proj":
            assert torch.equal(i16(v[:, :moe_gguf.I]), i16(q2[k][:, :moe_gguf.I]))
            assert torch.equal(i16(v[:, moe_gguf.I:]), i16(before[k][:, moe_gguf.I:]))
        else:
            assert torch.equal(i16(v), i16(before[k])), k
    assert [(ex.gate_up_proj.data_ptr(), ex.down_proj.data_ptr()) for ex in experts] == ptrs


@pytest.mark.parametrize("name", ["Q4_K", "Q8_0", "IQ4_XS"])
def test_packed_store_computes_what_the_packed_load_of_the_file_computes(world, name):
    from gptq_gguf_toolkit_amd import gguf_loader
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts
    model = moe_gguf.load_hf(world["hf"])
    free0 = torch.cuda.memory_allocated()
    store = LevelStore(model, world["db"], "cuda", MDB.UNITS + MDB.ATTENTION, resident="packed")
    dense = 2 * moe_gguf.LAYERS * 3 * moe_gguf.E * moe_gguf.I * moe_gguf.H
    assert store.freed_bytes >= dense and all(isinstance(model.model.layers[n].mlp.experts, PackedExperts) for n in range(moe_gguf.LAYERS))
    assert torch.cuda.memory_allocated() - free0 < store.bytes()  # the dense parameters are gone
    assert store.switch(MDB.uniform_state("Q2_K")) == len(MDB.UNITS) + len(MDB.ATTENTION)
    assert store.switch(MDB.uniform_state(name)) == len(MDB.UNITS) + len(MDB.ATTENTION) and store.jobs_issued == 0  # no launch
    ref = gguf_loader.load_into_model(moe_gguf.load_hf(world["hf"]), world["files"][name], packed=True)
    ids = world["ids"][0].cuda()
    with torch.no_grad():
        got, want = model(ids).logits, ref(ids).logits
    assert tuple(got.shape) == (1, 64, moe_gguf.V) and bool(torch.isfinite(got).all())
    assert torch.equal(i16(got), i16(want))


# ------------------------------------------------------------------------------------------------ the search
# With this seed three of the first generation's four offspring differ from the parent in block 1 only (first changed blocks
# 1, 0, 1, 1): the first stage saves more block forwards than the capture costs, so it runs from the cached boundary
# (suffix_forward.plan_stage) -- on two blocks most seeds never do.
SEED = "33"


def search_argv(world, db, trace, report, reuse):
    return ["--model_name_or_path", world["hf"], "--dtype", "float16", "--attn_implementation", "eager", "--calibration_data",
            world["ids_pt"], "--eval_datasets", world["ids_pt"], "--calibration_tokens", "512", "--eval_tokens", "192",
            "--calibration_sequence_length", "64", "--eval_sequence_length", "64", "--generations", "2", "--offspring", "4",
            "--target_bitwidth", "5", "--quant_weights_path", str(db), "--survivors_per_selection", "2", "1",
            "--tokens_per_selection", "128", "256", "--fitness_fn", "kl", "--resident", "dense", "--seed", SEED, "--reuse_prefix",
            reuse, "--trace_out", str(trace), "--report_out", str(report)]


def test_search_on_the_tiny_mixtral(world, tmp_path):
    import shutil
    from gptq_gguf_toolkit_amd import evo_quant_search as S, gguf_loader, ppleval
    from gptq_gguf_toolkit_amd.gguf_stitcher import stitch_search_result
    runs = {}
    for tag, reuse in (("a", "off"), ("b", "off"), ("r", "on")):
        db = tmp_path / tag
        shutil.copytree(world["db"], db)
        with redirect_stdout(io.StringIO()) as out:
            parent, cfg = S.main(search_argv(world, db, tmp_path / f"{tag}.json", tmp_path / f"{tag}-report.json", reuse))
        runs[tag] = dict(db=db, parent=parent, cfg=cfg, text=open(cfg).read(), trace=json.load(open(tmp_path / f"{tag}.json")),
                         report=json.load(open(tmp_path / f"{tag}-report.json")), out=out.getvalue())
    a = runs["a"]
    assert len(a["trace"]) == 2 and all(len(rec["offspring"]) == 4 for rec in a["trace"])
    assert runs["b"]["trace"] == a["trace"] and runs["b"]["text"] == a["text"]      # the run repeats
    assert runs["r"]["trace"] == a["trace"] and runs["r"]["text"] == a["text"]      # and --reuse_prefix on keeps it, bit for bit
    reused = [line for line in runs["r"]["out"].split("\n") if line.startswith("reuse_prefix:")]
    print(reused)
    assert len(reused) == 1 and not reused[0].startswith("reuse_prefix: 0 of")  # a Mixtral block ran from a cached boundary
    # the final configuration: units among its lines, within the budget
    lines = dict(line.split(": ", 1) for line in a["text"].split("\n"))
    assert set(lines) == set(MDB.UNITS + MDB.ATTENTION) and os.path.basename(a["cfg"]) == "evo-kl-configuration-5.0.txt"
    numel = {n: moe_gguf.E * moe_gguf.I * moe_gguf.H for n in MDB.UNITS}
    numel.update({n: moe_gguf.H * (moe_gguf.H if n.endswith(("q_proj", "o_proj")) else moe_gguf.H // 2) for n in MDB.ATTENTION})
    bits = sum(numel[n] * float(v.split()[0]) for n, v in lines.items())
    assert bits <= sum(int(numel[n] * 5.0) for n in lines)
    # ... stitched, verified, and read back
    gguf = stitch_search_result(str(a["db"]), a["cfg"], str(tmp_path / "mixed.gguf"), original_model=world["files"]["Q4_K"], verify=True)
    sd = gguf_loader.load_state_dict(str(gguf), "cuda", F16)
    assert tuple(sd["model.layers.1.mlp.experts.gate_up_proj"].shape) == (moe_gguf.E, 2 * moe_gguf.I, moe_gguf.H)
    # ppleval --gguf on the stitched file: the perplexity the search reported for its final state (same dtype, attention
    # implementation and dense weights; the sequences of --eval_tokens 192)
    res = tmp_path / "ppl.json"
    with redirect_stdout(io.StringIO()):
        ppleval.main(["--model_name_or_path", world["hf"], "--eval_datasets", world["ids_pt"], "--sequence_length", "64", "--eval_tokens",
                      "192", "--dtype", "float16", "--attn_implementation", "eager", "--gguf", str(gguf), "--output_file", str(res)])
    got = json.loads(res.read_text())["perplexity_results"][world["ids_pt"]]
    want = a["report"][f"ppl_eval/{world['ids_pt']}"]
    print(f"ppleval --gguf on the stitched file: {got!r}; the search's report of its final state: {want!r}")
    assert got == want
    assert a["report"]["train_fitness"] == a["trace"][-1]["stages"][-1]["fitnesses"][a["trace"][-1]["stages"][-1]["survivor_ids"][0]]
