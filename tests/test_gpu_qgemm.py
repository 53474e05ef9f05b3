"""The packed-weight forward on the GPU: gq_linear_packed (K21) against the block decoder and against fp64, its binding's
refusals, and packed residency -- PackedLinear, LevelStore(resident="packed"), the search, the .gguf loader -- on the tiny
Llama.  Weights are quantized random-normal matrices (finite decodes: a GEMM multiplies zeros of x with every weight)."""
import copy
import json
import os
import random
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from ggml_spec import TS
from test_gpu_decode import bits, gguf_model  # noqa: F401  (gguf_model: the fixture that builds the small .gguf)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

Q2, Q3, Q4, Q5, Q6, Q8 = 10, 11, 12, 13, 14, 8
TYPES = (Q2, Q3, Q4, Q5, Q6, Q8)
F16, BF16 = torch.float16, torch.bfloat16
GUARD = 64  # elements before and after y
FILL = 0x5A5A
ROW_BYTES = lambda t, C: C // 32 * 34 if t == Q8 else C // 256 * TS[t]  # noqa: E731


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from gptq_gguf_toolkit_amd import ops as _ops
    return _ops


def packed_weight(ops, t, R, C, seed, scale=1.0, offset=0, gather=False):
    """A seeded N(0, scale^2) matrix quantized to type t -> (1-D uint8 view of exactly the blocks' bytes at `offset` inside
    its buffer, row_src or None)."""
    W = (torch.randn(R, C, generator=torch.Generator().manual_seed(seed)) * scale).cuda()
    packed = ops.quantize_q8_0(W) if t == Q8 else ops.pack(t, *ops.rtn_quantize(W, t))
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (R, ROW_BYTES(t, C))
    n = packed.numel()
    buf = torch.zeros(offset + n + 16, dtype=torch.uint8, device="cuda")
    src = buf[offset:offset + n]
    src.copy_(packed.reshape(-1))
    assert src.data_ptr() % 16 == offset
    rows = torch.randperm(R, generator=torch.Generator().manual_seed(seed + 1)).to(torch.int32).cuda() if gather else None
    return src, rows


def subnormal(w):
    return (w != 0) & (w.float().abs() < torch.finfo(w.dtype).tiny)


# ------------------------------------------------------------------------------------------------ 1: x = I gives the decoder
# (type, R, C, byte offset of the source, row gather): Q3_K / Q6_K / Q8_0 at +2 (2-byte aligned, not 4), one K-quant and Q8_0
# gathered; [5, 768]: three superblocks per row, R no multiple of any tile; [130, 256]: a row tile plus two rows.
# Seeds 1000 + t + R: tests/ggml_spec.py's decoder on the oracle's RTN of these matrices yields no fp16 / bf16 subnormal at all.
IDENTITY = [(Q2, 5, 768, 0, False), (Q3, 5, 768, 2, False), (Q4, 5, 768, 0, True), (Q5, 5, 768, 0, False),
            (Q6, 5, 768, 2, False), (Q8, 5, 768, 2, True), (Q5, 130, 256, 0, False)]


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("t,R,C,off,gather", IDENTITY, ids=[f"q{c[0]}-{c[1]}x{c[2]}" for c in IDENTITY])
def test_identity_activations_reproduce_the_decoder(ops, t, R, C, off, gather, dt):
    src, rows = packed_weight(ops, t, R, C, seed=1000 + t + R, offset=off, gather=gather)
    want = ops.dequantize_blocks(t, src.view(R, -1), dt, rows)
    y = ops.linear_packed(t, src, torch.eye(C, dtype=dt, device="cuda"), rows)
    assert y.shape == (C, R) and y.dtype == dt
    sub = subnormal(want)  # the guides do not say whether the matrix pipe keeps 16-bit subnormal operands: left out
    n_sub = int(sub.sum())
    print(f"q_type {t} {dt}: {n_sub} subnormal expected values of {want.numel()}, "
          f"{int((y.T[sub] != want[sub]).sum())} of them differ")
    assert n_sub <= 0.01 * want.numel()
    assert bool(torch.isfinite(want).all())
    assert torch.equal(y.T[~sub], want[~sub]), f"{int((y.T != want)[~sub].sum())} of {want.numel()} values differ"


# ------------------------------------------------------------------------------------------------ 2: random x against fp64
GRID = [(T, R, C) for T in (1, 17, 129) for R in (1, 130) for C in (256, 2816)]  # 2816: 11 superblocks, an odd K loop
FP64 = [(T, R, C, TYPES[i % 6], (F16, BF16)[(i + i // 6) % 2]) for i, (T, R, C) in enumerate(GRID)]  # every type in both dtypes


def raw_call(t, src, rows, R, C, x, T, y):
    from gptq_gguf_toolkit_amd import _cabi
    from gptq_gguf_toolkit_amd.ops import _DT, _ptr, _stream
    _cabi.check(_cabi.lib().gq_linear_packed(t, _ptr(src), _ptr(rows), R, C, _ptr(x), T, _DT[x.dtype], _ptr(y), _stream(x)),
                "gq_linear_packed")


def guarded_y(T, R, dt):
    buf = torch.empty(T * R + 2 * GUARD, dtype=dt, device="cuda")
    bits(buf).fill_(FILL)
    return buf, buf[GUARD:GUARD + T * R].view(T, R)


def guards_intact(buf):
    iv = bits(buf)
    return bool((iv[:GUARD] == FILL).all()) and bool((iv[-GUARD:] == FILL).all())


# The library takes its 256-token tile from 512 workgroups of [256, 128] on, its 128-token tile below: [3850, 4090] is 16 x 32 =
# 512 of them (the last row tile and the last token tile cut), [3840, 4090] is 480.  Every type on the wide path, one beside it.
WIDE = [(3850, 4090, 256, t, (F16, BF16)[i % 2]) for i, t in enumerate(TYPES)] + [(3840, 4090, 256, Q4, F16)]
CASES = FP64 + WIDE


@pytest.mark.parametrize("T,R,C,t,dt", CASES, ids=[f"T{c[0]}-R{c[1]}-C{c[2]}-q{c[3]}-{str(c[4])[6:]}" for c in CASES])
def test_random_activations_against_fp64(ops, T, R, C, t, dt):
    """|y - y64| <= u |y64| + C 2^-23 (|x| |Wd|^T) + 2^-25 per element: the final rounding (u = 2^-11 fp16, 2^-8 bf16) plus the
    worst-case fp32 accumulation of C terms, doubled for a non-nearest internal add.  Derived, not measured."""
    src, rows = packed_weight(ops, t, R, C, seed=2000 + t + R + C, scale=0.02, gather=(R > 1 and t in (Q3, Q8)))
    x = torch.randn(T, C, generator=torch.Generator().manual_seed(T + C)).to(dt).cuda()
    Wd = ops.dequantize_blocks(t, src.view(R, -1), dt, rows)
    buf, y = guarded_y(T, R, dt)
    raw_call(t, src, rows, R, C, x, T, y)
    y64 = x.double() @ Wd.double().T
    u = 2.0 ** -11 if dt == F16 else 2.0 ** -8
    bound = u * y64.abs() + C * 2.0 ** -23 * (x.double().abs() @ Wd.double().abs().T) + 2.0 ** -25
    err = (y.double() - y64).abs()
    worst = float((err / bound).max())
    print(f"T={T} R={R} C={C} q_type {t} {dt}: max err / bound = {worst:.3f}")
    assert guards_intact(buf), "written outside [y, y + T * R * 2)"
    assert bool((err <= bound).all()), f"max err / bound = {worst}"
    if T > 1000:  # the wide path repeats itself too (test 3 is on the other one)
        again = ops.linear_packed(t, src, x, rows)
        assert torch.equal(bits(again), bits(y))


# ------------------------------------------------------------------------------------------------ 3: determinism
def test_the_same_call_gives_the_same_bits(ops):
    T, R, C = 129, 130, 2816
    src, rows = packed_weight(ops, Q4, R, C, seed=3000, scale=0.02)
    x = torch.randn(T, C, generator=torch.Generator().manual_seed(3)).half().cuda()
    a, b = ops.linear_packed(Q4, src, x), ops.linear_packed(Q4, src, x)
    assert torch.equal(bits(a), bits(b)) and bool(torch.isfinite(a).all()) and float(a.float().abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 4: the binding's refusals
def test_linear_packed_binding_refusals(ops):
    from gptq_gguf_toolkit_amd import _cabi
    src, _ = packed_weight(ops, Q4, 4, 256, seed=4000)
    x = torch.zeros(3, 256, dtype=F16, device="cuda")
    for args, word in (((Q4, src[:100], x), "144 bytes"),                                     # wrong byte count
                       ((Q4, src.view(2, -1), x), "144 bytes"),                               # rows of the wrong width
                       ((Q8, src, x), "272 bytes"),                                           # the bytes of another type
                       ((Q4, src, x.float()), "fp16 or bf16"),                                # fp32 x
                       ((Q4, src, x.cpu()), "CPU"),                                           # x on another device than blocks
                       ((Q4, src, torch.zeros(3, 512, dtype=F16, device="cuda")[:, ::2]), "contiguous"),
                       ((Q4, src, x, torch.zeros(3, dtype=torch.int32, device="cuda")), "row_src"),
                       ((Q4, src, torch.zeros(3, 128, dtype=F16, device="cuda")), "C=128")):
        with pytest.raises(_cabi.GQError, match=word):
            ops.linear_packed(*args)
    if torch.cuda.device_count() > 1:
        with pytest.raises(_cabi.GQError, match="one device"):
            ops.linear_packed(Q4, src, x.to("cuda:1"))
    assert ops.linear_packed(Q4, src, x.view(1, 3, 256)).shape == (1, 3, 4)                   # any leading shape


# ------------------------------------------------------------------------------------------------ 5: packed residency
LEVELS = ((Q2, "2"), (Q4, "4"), (Q6, "6"), (Q8, "8.5"))
LINEARS = r"((q|k|v|o|gate|up|down)_proj)$"


@pytest.fixture(scope="module")
def world(ops, tmp_path_factory):
    """The tiny Llama (hidden 256, 2 layers, vocab 512) in fp16 and four levels per Linear -- RTN Q2_K / Q4_K / Q6_K and Q8_0
    -- as a --gguf-layers database (gg/<tensor name>/<n>.pth + -metadata.json, manifest), as test_gpu_search.py's `world`."""
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd import metrics
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import map_tensor_name
    tmp = tmp_path_factory.mktemp("qgemm")
    model = tiny_llama(dtype=F16).cuda()
    names = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and re.search(LINEARS, n)]
    assert len(names) == 14
    for n in names:
        W = model.get_submodule(n).weight.data
        g = map_tensor_name(n + ".weight")
        (tmp / "gg" / g).mkdir(parents=True)
        for t, num in LEVELS:
            packed = ops.quantize_q8_0(W) if t == Q8 else ops.pack(t, *ops.rtn_quantize(W, t))
            packed.cpu().numpy().tofile(str(tmp / "gg" / g / f"{num}.pth"))
            (tmp / "gg" / g / f"{num}-metadata.json").write_text(json.dumps({"tensor_info": {
                "name": g, "type": t, "shape": [W.shape[1], W.shape[0]], "np_shape": list(packed.shape), "np_dtype": "uint8"}}))
    md = {"general.architecture": {"value": "llama"}, "llama.attention.head_count": {"value": 4},
          "llama.attention.head_count_kv": {"value": 2}}
    (tmp / "gg" / "manifest.json").write_text(json.dumps({"metadata": md}))
    calib = tiny_calib()
    targets = metrics.collect_target_logits(model, calib)  # the unmodified dense model
    return model, names, str(tmp / "gg"), calib, targets


def mixed_state(names):
    keys = [k for _, k in LEVELS]
    return {n: float(keys[(3 * i + 1) % 4]) for i, n in enumerate(names)}


def test_packed_store_holds_no_dense_weight_and_switches_by_reference(world):
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    base, names, db, _, _ = world
    dense_model, model = copy.deepcopy(base), copy.deepcopy(base)
    dense_bytes = sum(model.get_submodule(n).weight.numel() * 2 for n in names)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    store = LevelStore(model, db, "cuda", resident="packed")
    after = torch.cuda.memory_allocated()
    numel = dense_bytes // 2
    assert store.freed_bytes == dense_bytes and list(store.layers) == names
    assert numel * (84 + 144 + 210 + 272) // 256 <= store.bytes() <= numel * (84 + 144 + 210 + 272) // 256 + 4 * (256 + 128)
    # the arithmetic, in the allocator's 512-byte granules (a Q6_K level of a [128, 256] Linear is 52.5 of them): the dense
    # weights went, every level and every row index came, nothing else moved
    granules = lambda n: -(-n // 512) * 512  # noqa: E731
    held = (sum(granules(lv.nbytes) for lvs in store.levels.values() for lv in lvs) +
            sum(granules(r.numel() * 4) for r in store._rows.values() if r is not None))
    assert store.bytes() <= held < store.bytes() + 512 * 4 * len(names)
    assert before - after == dense_bytes - held, (before, after, dense_bytes, held, store.bytes())
    for n in names:
        m = model.get_submodule(n)
        assert type(m) is PackedLinear and m.weight.device.type == "meta" and not list(m.parameters())
        assert m.weight.shape == base.get_submodule(n).weight.shape and m.weight.numel() == m.in_features * m.out_features
    assert not any(p.dim() == 2 and n.rsplit(".", 1)[0] in names for n, p in model.named_parameters())

    dense = LevelStore(dense_model, db, "cuda")
    state = mixed_state(names)
    assert len(set(state.values())) == 4
    m0 = torch.cuda.memory_allocated()
    assert store.switch(state) == 14
    assert torch.cuda.memory_allocated() == m0 and store.jobs_issued == 0
    assert dense.switch(state) == 14 and dense.jobs_issued == 14
    for n in names:
        m, lv = model.get_submodule(n), store.find(n, state[n])
        assert m.blocks.data_ptr() == lv.data.data_ptr() and m.q_type == lv.kind and m.row_src is lv.rows, n
        assert torch.equal(bits(m.dense_weight()), bits(dense_model.get_submodule(n).weight.data)), n
    assert model.get_submodule("model.layers.0.self_attn.q_proj").row_src is not None      # q / k: the rotary row gather
    assert model.get_submodule("model.layers.0.mlp.up_proj").row_src is None
    flipped = dict(state)
    flipped[names[0]], flipped[names[5]] = 8.5 if state[names[0]] != 8.5 else 2.0, 6.0 if state[names[5]] != 6.0 else 4.0
    assert store.switch(flipped) == 2 and store.switch(flipped) == 0 and store.jobs_issued == 0
    assert torch.cuda.memory_allocated() == m0
    assert torch.equal(bits(store.weight_of(names[0], flipped[names[0]])), bits(model.get_submodule(names[0]).dense_weight()))
    assert store.level_tensor(names[5], flipped[names[5]]).dtype == F16


def test_packed_fitness_equals_dense_fitness_within_the_forward_rounding(world):
    """KL against the dense model's targets, packed versus dense residency.  The yardstick is torch's own forward:
    floor = |KL(dense, fp16 forward) - KL(same weights, model and inputs in fp32)|, the rounding noise of the 16-bit forward
    itself; the packed path differs from dense only in fp32 summation order."""
    from gptq_gguf_toolkit_amd import metrics
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    base, names, db, calib, targets = world
    dense_model, model = copy.deepcopy(base), copy.deepcopy(base)
    state = mixed_state(names)
    LevelStore(dense_model, db, "cuda").switch(state)
    LevelStore(model, db, "cuda", resident="packed").switch(state)
    kl_dense = metrics.compute_kl_div(dense_model, calib, targets)
    kl_packed = metrics.compute_kl_div(model, calib, targets)
    kl_fp32 = metrics.compute_kl_div(copy.deepcopy(dense_model).float(), calib, targets)
    floor = abs(kl_dense - kl_fp32)
    msg = f"KL packed {kl_packed!r}, dense {kl_dense!r}, the same weights in fp32 {kl_fp32!r} (floor {floor!r})"
    print(msg)
    assert np.isfinite(kl_packed) and kl_packed > 0, msg
    assert abs(kl_packed - kl_dense) <= floor, msg


def test_search_on_a_packed_store(world):
    from gptq_gguf_toolkit_amd import evo_quant_search as S
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    base, names, db, calib, targets = world
    model = copy.deepcopy(base)
    levels = S.scan_available_bitwidths(db, names)
    assert all([bw for bw, _ in v] == [2.0, 4.0, 6.0, 8.5] for v in levels.values())
    grouped = S.group_layers(model, sorted(levels, key=S.layer_order_fn), "size")
    store = LevelStore(model, db, "cuda", [n for g in grouped for n in g], resident="packed")
    store.grouped_layer_names = grouped
    ctx = S._Ctx(model, grouped, levels, S.target_bits_of(grouped, model, 4.0))  # the accounting reads the meta weights
    assert ctx.target_bits == 4 * sum(base.get_submodule(n).weight.numel() for n in names)

    def evaluate(candidate, data, tg):
        store.switch(candidate)
        return S.compute_fitness(model, data, "kl", tg)

    parent, fit, trace = S.search(ctx, evaluate, calib, random.Random(0), generations=3, offspring=6, target_bitwidth=4.0,
                                  survivors_per_selection=(2, 1), tokens_per_selection=(128, 256), group_rule="size",
                                  fitness_fn="kl", target_logits=targets)
    assert len(trace) == 3 and ctx.bits(parent) <= ctx.target_bits and store.jobs_issued == 0
    assert np.isfinite(fit) and fit > 0
    for rec in trace:
        assert all(np.isfinite(f) and f > 0 for st in rec["stages"] for f in st["fitnesses"])


def test_gguf_file_loads_packed(gguf_model):  # noqa: F811
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd import gguf_loader
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    _, path = gguf_model
    dense = gguf_loader.load_into_model(tiny_llama(seed=123, dtype=F16).cuda(), path)
    packed = gguf_loader.load_into_model(tiny_llama(seed=321, dtype=F16).cuda(), path, packed=True)
    names = [n for n, m in dense.named_modules() if isinstance(m, torch.nn.Linear) and re.search(LINEARS, n)]
    assert len(names) == 14
    for n in names:
        m = packed.get_submodule(n)
        assert type(m) is PackedLinear and m.q_type in TYPES, n
        assert (m.row_src is not None) == n.endswith(("q_proj", "k_proj")), n   # q / k come through the row gather
        assert torch.equal(bits(m.dense_weight()), bits(dense.get_submodule(n).weight.data)), n
    assert type(packed.lm_head) is torch.nn.Linear  # embeddings, norms and lm_head load as without the flag
    for k, w in packed.state_dict().items():
        assert torch.equal(bits(w), bits(dense.state_dict()[k])), k
    ids = tiny_calib()[0].cuda()
    with torch.no_grad():
        got, want = packed(ids).logits, dense(ids).logits
    print(f"logits, packed against dense: max |difference| {float((got.float() - want.float()).abs().max())!r} "
          f"of max |logit| {float(want.float().abs().max())!r}")
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
