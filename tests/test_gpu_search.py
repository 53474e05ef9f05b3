"""-m gpu: K18, the level switch of the bit-width search -- gq_level_switch through ops.level_switch, LevelStore on both
database layouts, and evo_quant_search.search on the tiny Llama.  Every weight equality is on bits.  Anchors: the package's
ops.dequantize_blocks (pinned to the reference by G6-G9), the independent ggml-layout decoder tests/ggml_spec.py, torch's
.to(dtype), and level_db.load_level (the reference's load path)."""
import copy
import json
import os
import random
import sys

import numpy as np
import pytest

from conftest import ROOT
from ggml_spec import TS, unpack as spec_unpack
from test_gpu_decode import bits, formula_f32, random_blocks

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

Q2, Q3, Q4, Q5, Q6 = 10, 11, 12, 13, 14
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
GUARD = 64  # elements before and after every destination


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from gptq_gguf_toolkit_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------ the kernel
# (q_type, R, blocks per row, byte offset of the source inside its buffer, row gather?) -- 1, 15, 16, 17 and 33 blocks
PACKED = {"Q4_K 1x256": (Q4, 1, 1, 0, False), "Q2_K 5x768": (Q2, 5, 3, 0, False), "Q5_K 2x2048": (Q5, 2, 8, 0, False),
          "Q3_K 17x256 gathered, at +2": (Q3, 17, 1, 2, True), "Q6_K 3x2816, at +6": (Q6, 3, 11, 6, False)}


@pytest.fixture(scope="module")
def specs(ops):
    """The job kinds of the kernel test, each with its source on the device and its expected result (computed once):
    name -> (src, kind, row_src, (R, C), out dtype, expected)."""
    out = {}
    for name, (t, R, nb, off, gather) in PACKED.items():
        raw = random_blocks(t, R, nb, seed=100 + t)
        buf = torch.zeros(off + raw.size + 16, dtype=torch.uint8, device="cuda")
        src = buf[off:off + raw.size]
        src.copy_(torch.from_numpy(raw.reshape(-1)))
        assert src.data_ptr() % 16 == off  # +2 / +6: 2-byte aligned and not 4-byte aligned
        rows = torch.randperm(R, generator=torch.Generator().manual_seed(t)).to(torch.int32).cuda() if gather else None
        want32 = formula_f32(t, spec_unpack(t, raw))  # tests/ggml_spec.py, numpy fp32
        if rows is not None:
            want32 = want32[rows.cpu().long().numpy()]
        for dt in (F32, F16, BF16):
            if dt == BF16 and t != Q6:
                continue  # every type -> fp32 and fp16; Q6_K also -> bf16
            exp = ops.dequantize_blocks(t, src.view(R, nb * TS[t]), dt, rows)
            assert torch.equal(bits(exp).cpu(), bits(torch.from_numpy(want32).to(dt))), (name, dt)
            out[f"{name} -> {dt}"] = (src, t, rows, (R, nb * 256), dt, exp)
    g = torch.Generator().manual_seed(9)
    a = (torch.randn(7, 264, generator=g) * 3).half().cuda()
    out["dense fp16 -> bf16 7x264"] = (a, None, None, (7, 264), BF16, a.to(BF16))
    b = (torch.randn(5, 72, generator=g) * 100).cuda()
    b[0, :4] = torch.tensor([65520.0, 1e-8, -0.0, 6.1e-5])  # overflow to inf, underflow, signed zero, a subnormal result
    rows = torch.tensor([3, 0, 4, 4, 1], dtype=torch.int32).cuda()
    out["dense fp32 -> fp16 5x72 gathered"] = (b, None, rows, (5, 72), F16, b[rows.long()].to(F16))
    c = (torch.randn(3, 8, generator=g)).to(BF16).cuda()
    out["dense bf16 -> fp32 3x8"] = (c, None, None, (3, 8), F32, c.to(F32))
    torch.cuda.synchronize()
    return out


def guarded(shape, dt):
    n = shape[0] * shape[1]
    buf = torch.empty(n + 2 * GUARD, dtype=dt, device="cuda")
    iv = bits(buf)
    iv.fill_(0x5A5A if dt != F32 else 0x5A5A5A5A)
    return buf, buf[GUARD:GUARD + n].view(shape)


def test_every_job_kind_in_one_call(ops, specs):
    """All kinds in ONE call: 1, 15, 16, 17 and 33 blocks, every type to fp32 and fp16, gathers, odd source offsets, dense."""
    names = list(specs)
    assert len(names) == 14
    bufs, jobs = [], []
    for n in names:
        src, kind, rows, shape, dt, _ = specs[n]
        buf, dst = guarded(shape, dt)
        bufs.append(buf)
        jobs.append((src, dst, kind, rows))
    assert ops.level_switch(jobs) is None
    for n, buf, (_, dst, _, _) in zip(names, bufs, jobs):
        exp, iv = specs[n][5], bits(buf)
        assert torch.equal(bits(dst), bits(exp)), n
        s = 0x5A5A if buf.dtype != F32 else 0x5A5A5A5A
        assert bool((iv[:GUARD] == s).all()) and bool((iv[-GUARD:] == s).all()), f"{n}: guard overwritten"


@pytest.mark.parametrize("n_jobs", [1, 64, 65])
def test_list_lengths_around_the_launch_limit(ops, specs, n_jobs):
    from gptq_gguf_toolkit_amd import _cabi
    assert _cabi.SWITCH_MAX_JOBS == 64
    names = list(specs)
    picks = [names[(5 * i + 3) % len(names)] for i in range(n_jobs)]  # job 64 (the second launch's only one) is packed
    bufs, jobs = [], []
    for n in picks:
        src, kind, rows, shape, dt, _ = specs[n]
        buf, dst = guarded(shape, dt)
        bufs.append(buf)
        jobs.append((src, dst, kind, rows))
    ops.level_switch(jobs)
    for i, (n, buf, job) in enumerate(zip(picks, bufs, jobs)):
        assert torch.equal(bits(job[1]), bits(specs[n][5])), (i, n)
        iv, s = bits(buf), 0x5A5A if buf.dtype != F32 else 0x5A5A5A5A
        assert bool((iv[:GUARD] == s).all()) and bool((iv[-GUARD:] == s).all()), (i, n)


def test_binding_refusals(ops, specs):
    from gptq_gguf_toolkit_amd import _cabi
    src, kind, rows, shape, dt, _ = specs["Q4_K 1x256 -> torch.float16"]
    dst = torch.empty(shape, dtype=dt, device="cuda")
    strided = torch.empty(1, 512, dtype=dt, device="cuda")[:, ::2]
    for bad, word in (((src, strided, kind, None), "contiguous"), ((src[:100], dst, kind, None), "144 uint8"),
                      ((src, dst, None, None), "dense src"), ((src, dst, kind, torch.zeros(3, dtype=torch.int32).cuda()), "row_src"),
                      ((src.cpu(), dst, kind, None), "CPU")):
        with pytest.raises(_cabi.GQError, match=word):
            ops.level_switch([bad])


# ------------------------------------------------------------------------------------------------ the store
LEVELS = ((Q2, "2", "Q2_K"), (Q4, "4", "Q4_K"), (Q6, "6", "Q6_K"))
LINEARS = r"((q|k|v|o|gate|up|down)_proj)$"


@pytest.fixture(scope="module")
def world(ops, tmp_path_factory):
    """The tiny Llama (hidden 256, 2 layers, vocab 512) in fp16 and three RTN levels per Linear in both database layouts:
    hf/<module name>/<n>-<Qn_K>.pth (dense fp16, torch.save) and gg/<tensor name>/<n>.pth (+ -metadata.json, manifest)."""
    import re
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import map_tensor_name
    tmp = tmp_path_factory.mktemp("search")
    model = tiny_llama(dtype=F16).cuda()
    names = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and re.search(LINEARS, n)]
    assert len(names) == 14
    for n in names:
        W = model.get_submodule(n).weight.data
        g = map_tensor_name(n + ".weight")
        (tmp / "hf" / n).mkdir(parents=True)
        (tmp / "gg" / g).mkdir(parents=True)
        for t, num, tag in LEVELS:
            packed = ops.pack(t, *ops.rtn_quantize(W, t))
            torch.save(ops.dequantize_blocks(t, packed, F16).cpu(), str(tmp / "hf" / n / f"{num}-{tag}.pth"))
            packed.cpu().numpy().tofile(str(tmp / "gg" / g / f"{num}.pth"))
            (tmp / "gg" / g / f"{num}-metadata.json").write_text(json.dumps({"tensor_info": {
                "name": g, "type": t, "shape": [W.shape[1], W.shape[0]], "np_shape": list(packed.shape), "np_dtype": "uint8"}}))
    md = {"general.architecture": {"value": "llama"}, "llama.attention.head_count": {"value": 4},
          "llama.attention.head_count_kv": {"value": 2}}
    (tmp / "gg" / "manifest.json").write_text(json.dumps({"metadata": md}))
    (tmp / "hf" / "manifest.json").write_text("{}")
    return model, names, tmp, tiny_calib()


@pytest.mark.parametrize("layout", ["hf", "gg"])
def test_store_switch_equals_the_reference_load_path(world, layout):
    from gptq_gguf_toolkit_amd import level_db as ldb
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    model, names, tmp, _ = world
    model = copy.deepcopy(model)
    db = str(tmp / layout)
    store = LevelStore(model, db, "cuda")
    assert list(store.layers) == names and all(store.level_keys(n) == [2.0, 4.0, 6.0] for n in names)
    per_param = {"hf": 3 * 2.0, "gg": (84 + 144 + 210) / 256}[layout]
    numel = sum(model.get_submodule(n).weight.numel() for n in names)
    assert numel * per_param <= store.bytes() <= numel * per_param + 4 * (256 + 128)  # the levels as stored (+ q / k row indices)
    ptrs = {n: model.get_submodule(n).weight.data_ptr() for n in names}

    def check(state):
        for n, key in state.items():
            ldir = ldb.layer_dir(db, n)
            f = next(f for f in ldb.level_files(ldir) if ldb.level_key(f) == key)
            want = ldb.load_level(os.path.join(ldir, f), "cuda", db).to(F16)
            w = model.get_submodule(n).weight
            assert torch.equal(bits(w.data), bits(want)), (n, key)
            assert w.data_ptr() == ptrs[n], n

    initial = {n: 4.0 for n in names}
    assert store.switch(initial) == 14
    check(initial)
    flipped = dict(initial)
    flipped[names[0]], flipped[names[5]], flipped[names[13]] = 2.0, 6.0, 2.0  # a 3-flip offspring
    assert store.switch(flipped) == 3                                         # only the diff is rewritten
    check(flipped)
    assert store.switch(flipped) == 0
    assert store.switch(initial) == 3
    check(initial)
    # q / k of the GGUF layout come through the rotary row gather: not the rows as stored
    if layout == "gg":
        q = names.index("model.layers.0.self_attn.q_proj")
        lv = store.find(names[q], 4.0)
        assert lv.rows is not None and lv.kind == Q4 and lv.data.dtype == torch.uint8
        assert store.find("model.layers.0.mlp.up_proj", 4.0).rows is None
        assert store.find("model.layers.1.self_attn.q_proj", 2.0).rows is lv.rows  # built once per shape


def test_store_refusals(world):
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    model, names, tmp, _ = world
    with pytest.raises(MemoryError, match=r"need \d+ bytes"):
        LevelStore(model, str(tmp / "gg"), "cuda", capacity_bytes=1000)
    other = copy.deepcopy(model)
    other.model.layers[0].mlp.up_proj = torch.nn.Linear(256, 256, bias=False).half().cuda()
    with pytest.raises(ValueError, match="has shape"):
        LevelStore(other, str(tmp / "gg"), "cuda")
    with pytest.raises(ValueError, match="has shape"):
        LevelStore(other, str(tmp / "hf"), "cuda")


def test_error_estimator_takes_the_store(world):
    from gptq_gguf_toolkit_amd import error_estimator as ee
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    model, names, tmp, calib = world
    model = copy.deepcopy(model)
    data = [([], {"input_ids": ids}) for ids in calib[:2]]
    args = (model, data, r".*layers.*" + LINEARS, ["model.embed_tokens"], "model.layers", str(tmp / "gg"))
    plain = ee.ErrorEstimator(*args, device="cuda:0").estimate()
    store = LevelStore(model, str(tmp / "gg"), "cuda")
    through = ee.ErrorEstimator(*args, device="cuda:0", level_store=store).estimate()
    assert dict(plain[-1]) == dict(through[-1]) and len(plain[-1]) == 14


# ------------------------------------------------------------------------------------------------ the search
def test_search_on_the_tiny_llama(world, tmp_path):
    from gptq_gguf_toolkit_amd import evo_quant_search as S, level_db as ldb, metrics, ppleval
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    base, names, tmp, calib = world
    db = str(tmp / "hf")
    model = copy.deepcopy(base)
    targets = metrics.collect_target_logits(model, calib)  # the unmodified model, on the device
    levels = S.scan_available_bitwidths(db)
    assert set(levels) == set(names) and all([bw for bw, _ in v] == [2.0, 4.0, 6.0] for v in levels.values())
    grouped = S.group_layers(model, sorted(levels, key=S.layer_order_fn), "size")
    store = LevelStore(model, db, "cuda", [n for g in grouped for n in g])
    store.grouped_layer_names = grouped
    ctx = S._Ctx(model, grouped, levels, S.target_bits_of(grouped, model, 4.0))

    def evaluate(candidate, data, tg):
        store.switch(candidate)
        return S.compute_fitness(model, data, "kl", tg)

    parent, fit, trace = S.search(ctx, evaluate, calib, random.Random(0), generations=3, offspring=6, target_bitwidth=4.0,
                                  survivors_per_selection=(2, 1), tokens_per_selection=(128, 256), group_rule="size",
                                  fitness_fn="kl", target_logits=targets)
    assert len(trace) == 3 and ctx.bits(parent) <= ctx.target_bits
    for rec in trace:  # elitism: on the last stage's minibatch the survivor is no worse than the parent
        last = rec["stages"][-1]
        assert last["candidates"][-1] == rec["parent"] and len(last["minibatch_ids"]) == 4
        assert last["fitnesses"][last["survivor_ids"][0]] <= last["fitnesses"][-1]
        assert all(np.isfinite(f) and f > 0 for st in rec["stages"] for f in st["fitnesses"])
    assert fit == trace[-1]["stages"][-1]["fitnesses"][trace[-1]["stages"][-1]["survivor_ids"][0]]

    # the written configuration loads through ppleval to the weights the store holds
    cfg = tmp_path / S.configuration_name("kl", 4.0)
    cfg.write_text(S.configuration_text(grouped, parent, levels))
    assert cfg.name == "evo-kl-configuration-4.0.txt" and not cfg.read_text().endswith("\n")
    store.switch(parent)
    loaded = ppleval.load_compressed_weights(copy.deepcopy(base), db, str(cfg))
    for n in names:
        assert torch.equal(bits(loaded.get_submodule(n).weight.data), bits(model.get_submodule(n).weight.data)), n

    # a candidate's fitness through the store against the reference's path (load_level + .to(dtype) + compute_kl_div)
    st = trace[1]["stages"][0]
    cand, got = st["candidates"][0], st["fitnesses"][0]
    assert cand != trace[1]["parent"]
    data, tg = [calib[i] for i in st["minibatch_ids"]], [targets[i] for i in st["minibatch_ids"]]
    ref = copy.deepcopy(base)
    for n, bw in store.flatten(cand).items():
        f = S.filename_of(levels, n, bw)
        layer = ref.get_submodule(n)
        layer.weight.data = ldb.load_level(os.path.join(db, n, f), "cuda", db).to(layer.weight.dtype)
    want = [metrics.compute_kl_div(ref, data, tg) for _ in range(2)]
    spread = abs(want[0] - want[1])
    print(f"fitness through the store {got!r}, through the reference's path {want[0]!r}, {want[1]!r} (spread {spread!r})")
    assert abs(got - want[0]) <= spread  # bit-identical weights: equality unless the GEMM itself does not repeat
    assert evaluate(cand, data, tg) == got or spread > 0
