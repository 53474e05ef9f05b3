"""The grouped prefill path of PackedExperts on the GPU, in the 2-layer Mixtral of tests/moe_gguf.py (4 experts, top-2; the six
packed types spread over the expert tensors of the two layers): the module against the spelled-out composition of its ops
calls and against fp64, the whole model against the loop path and the fp32 model, the launches it makes, that it makes no
host synchronisation (which the loop path does), and the defaults it leaves alone.  Fixtures, bounds and floors are
test_gpu_moe_model.py's."""
import io
import json
import math
from contextlib import redirect_stdout

import pytest

import moe_gguf
from test_gpu_moe_model import E, H, I, K, ROLE_FILE, fp64_and_bound, i16, routed, routing, world  # noqa: F401
from test_gpu_packed_vocab import N_PROMPT, incremental

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def grouped(world):  # noqa: F811
    """The same file loaded packed with moe_prefill="grouped"."""
    from gptq_gguf_toolkit_amd import gguf_loader
    return gguf_loader.load_into_model(moe_gguf.load_hf(world["hf"]), world["gguf"], packed=True, moe_prefill="grouped")


# ------------------------------------------------------------------------------------------------ the expert module alone
def composed(ex, x, idx, w):
    """The prefill path spelled out: ops.moe_route, then per expert ops.linear_packed on the slices of the three stacked
    tensors with the expert's tokens gathered by the route, ops.fwd_silu_mul, and the combine the decode path shares."""
    from gptq_gguf_toolkit_amd import ops
    sl = {r: (ex.levels[r][0].view(E, -1), ex.levels[r][1]) for r in ROLE_FILE}
    T = x.shape[0]
    pairs = idx.reshape(-1).to(torch.int32)
    start, order = ops.moe_route(pairs, E)
    start = start.tolist()
    gate, up = (torch.zeros(T * K, I, dtype=x.dtype, device="cuda") for _ in range(2))
    down = torch.full((T * K, H), float("nan"), dtype=x.dtype, device="cuda")
    runs = [order[start[e]:start[e + 1]].long() for e in range(E)]
    for e, run in enumerate(runs):
        if run.numel():
            cur = x[run // K].contiguous()
            gate[run] = ops.linear_packed(sl["gate"][1], sl["gate"][0][e], cur)
            up[run] = ops.linear_packed(sl["up"][1], sl["up"][0][e], cur)
    a = ops.fwd_silu_mul(gate, up)
    for e, run in enumerate(runs):
        if run.numel():
            down[run] = ops.linear_packed(sl["down"][1], sl["down"][0][e], a[run].contiguous())
    return ex._combine(down, pairs, w)


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("T", [40, 48])
def test_grouped_prefill_is_the_composition_of_its_calls(grouped, layer, T):
    """Bit for bit the composition above (gq_linear_packed_experts' contract, three times, and one shared combine), and within
    the bound test_gpu_moe_model.py composes for the three GEMMs against fp64."""
    ex = grouped.model.layers[layer].mlp.experts
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(10 * T + layer)).half().cuda()
    idx, w = routing(T, seed=T)
    assert ex.prefill == "grouped" and ex.takes_prefill_path(T, K) and not ex.takes_decode_path(T, K)
    with torch.no_grad():
        got = ex(x, idx, w)
        want = composed(ex, x, idx, w)
    assert got.shape == (T, H) and got.dtype == torch.float16 and bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    assert torch.equal(i16(got), i16(want)), int((i16(got) != i16(want)).sum())
    out64, B = fp64_and_bound(ex, x, idx, w)
    err = (got.double() - out64).abs()
    print(f"layer {layer} T={T}: grouped prefill err / B = {float((err / B).max()):.3f}")
    assert bool((err <= B).all())
    ex.prefill_max_pairs = 32  # chunks of 16 tokens: the same bits (a pair's result does not depend on the other pairs)
    try:
        with torch.no_grad():
            parts = ex(x, idx, w)
    finally:
        del ex.prefill_max_pairs
    assert torch.equal(i16(parts), i16(got))


# ------------------------------------------------------------------------------------------------ the whole model
def test_whole_model_routes_as_the_loop_path_and_scores_within_the_noise(world, grouped):  # noqa: F811
    """48 tokens through the whole model: the router decisions of both layers are the loop path's, and with
    test_gpu_moe_model.py's floor (max |dense fp16 - fp32| over the same logits; ln ppl is 2-Lipschitz in the largest logit
    difference and the packed logits are held to 2 floor) |ln ppl(grouped) - ln ppl(fp32)| <= 4 floor."""
    data = world["ids"][0][:, :48].cuda()
    r_loop, l_loop = routed(world["packed"], data)
    r_grouped, l_grouped = routed(grouped, data)
    flips = [int((a != b).any(-1).sum()) for a, b in zip(r_loop, r_grouped)]
    assert len(r_grouped) == moe_gguf.LAYERS and r_grouped[0].shape == (48, K) and flips == [0] * moe_gguf.LAYERS, flips
    with torch.no_grad():
        ref = world["fp32"](data).logits
        l_dense = world["dense"](data).logits

    def ln_ppl(logits):
        return float(torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, moe_gguf.V).double(), data[:, 1:].reshape(-1)))

    floor = float((l_dense.float() - ref).abs().max())
    err = float((l_grouped.float() - ref).abs().max())
    print(f"48 tokens: ln ppl grouped {ln_ppl(l_grouped)!r}, loop {ln_ppl(l_loop)!r}, fp32 {ln_ppl(ref)!r}; floor {floor!r}; "
          f"grouped logits against fp32 {err!r}")
    assert floor > 0 and bool(torch.isfinite(l_grouped).all())
    assert abs(ln_ppl(l_grouped) - ln_ppl(ref)) <= 4 * floor


def test_ppleval_command_line_takes_the_choice(world):  # noqa: F811
    from test_gpu_eval import run_ppleval
    from gptq_gguf_toolkit_amd import metrics
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts
    res, scored = run_ppleval(world, "moe_grouped", "--gguf", world["gguf"], "--packed", "--moe_prefill", "grouped")
    assert all(type(layer.mlp.experts) is PackedExperts and layer.mlp.experts.prefill == "grouped" for layer in scored.model.layers)
    ppl = res["perplexity_results"][world["ids_pt"]]
    rows = metrics.nll_rows(scored, world["ids"])  # the command line reproduces the API's number on the model it describes
    assert math.isfinite(ppl) and abs(ppl / math.exp(float(rows.double().mean())) - 1) < 1e-12


# ------------------------------------------------------------------------------------------------ launches, synchronisation
def test_prefill_launches_one_route_and_three_grouped_gemms_per_layer_and_chunk(grouped, world, monkeypatch):  # noqa: F811
    from gptq_gguf_toolkit_amd import ops
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts
    calls = {"route": 0, "grouped": 0, "linear_in_experts": 0, "gemv_in_experts": 0, "inside": False}
    real = {n: getattr(ops, n) for n in ("moe_route", "linear_packed_experts", "linear_packed", "gemv_packed")}
    real_f = PackedExperts.forward

    def counted(name, key):
        def fn(*a, **k):
            if key.endswith("_in_experts"):
                calls[key] += calls["inside"]
            else:
                calls[key] += 1
            return real[name](*a, **k)
        return fn

    def forward(self, *a, **k):
        calls["inside"] = True
        try:
            return real_f(self, *a, **k)
        finally:
            calls["inside"] = False

    monkeypatch.setattr(ops, "moe_route", counted("moe_route", "route"))
    monkeypatch.setattr(ops, "linear_packed_experts", counted("linear_packed_experts", "grouped"))
    monkeypatch.setattr(ops, "linear_packed", counted("linear_packed", "linear_in_experts"))
    monkeypatch.setattr(ops, "gemv_packed", counted("gemv_packed", "gemv_in_experts"))
    monkeypatch.setattr(PackedExperts, "forward", forward)
    data = world["ids"][1][:, :48].cuda()
    with torch.no_grad():
        grouped(data)
    assert (calls["route"], calls["grouped"]) == (moe_gguf.LAYERS, 3 * moe_gguf.LAYERS)
    assert calls["linear_in_experts"] == 0 and calls["gemv_in_experts"] == 0
    experts = [layer.mlp.experts for layer in grouped.model.layers]
    for ex in experts:
        ex.prefill_max_pairs = 32  # 16 tokens a chunk: three chunks
    try:
        with torch.no_grad():
            grouped(data)
    finally:
        for ex in experts:
            del ex.prefill_max_pairs
    assert (calls["route"], calls["grouped"]) == (4 * moe_gguf.LAYERS, 12 * moe_gguf.LAYERS)
    assert calls["linear_in_experts"] == 0 and calls["gemv_in_experts"] == 0


def test_grouped_prefill_makes_no_host_synchronisation_and_the_loop_path_does(world, grouped):  # noqa: F811
    """The whole-model forward of 48 tokens under torch's synchronisation check.  The causal mask is an input here, prepared
    ahead in the 4-D form transformers passes through as it is: its own mask factory fills the mask from a host scalar, a
    copy the check counts, and that is not the experts' business."""
    data = world["ids"][2][:, :48].cuda()
    mask = torch.full((1, 1, 48, 48), torch.finfo(torch.float16).min, dtype=torch.float16, device="cuda").triu(1)
    ex_loop = world["packed"].model.layers[0].mlp.experts
    x = torch.randn(40, H, generator=torch.Generator().manual_seed(1)).half().cuda()
    idx, w = routing(40, seed=1)
    with torch.no_grad():
        want = grouped(data, attention_mask=mask).logits  # (and whatever the first forward of a model sets up)
    probe = torch.ones(4, device="cuda")
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    loop_raised = None
    try:
        try:
            probe.nonzero()
            control = False
        except RuntimeError:
            control = True
        if control:
            with torch.no_grad():
                got = grouped(data, attention_mask=mask).logits
                try:
                    ex_loop(x, idx, w)
                    loop_raised = False
                except RuntimeError:
                    loop_raised = True
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    if not control:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .nonzero() raise on this build")
    assert torch.equal(i16(got), i16(want))
    assert loop_raised, "the loop path no longer synchronises: this test's contrast is gone"


# ------------------------------------------------------------------------------------------------ defaults, generate
def test_the_default_stays_the_loop_and_generate_gives_the_same_greedy_tokens(world, grouped):  # noqa: F811
    from gptq_gguf_toolkit_amd import generate
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts
    for layer in world["packed"].model.layers:  # load_into_model(..., packed=True) without the keyword
        assert type(layer.mlp.experts) is PackedExperts and layer.mlp.experts.prefill == "loop"
        assert "prefill" not in vars(layer.mlp.experts)
    assert PackedExperts.prefill == "loop"
    out = world["tmp"] / "gen_grouped.json"
    argv = ["--model_name_or_path", world["hf"], "--gguf", world["gguf"], "--packed", "--moe_prefill", "grouped", "--prompt_ids",
            world["ids_pt"], "--max_new_tokens", "4", "--dtype", "float16", "--attn_implementation", "eager", "--output_file", str(out)]
    with redirect_stdout(io.StringIO()):
        generate.main(argv)
    res = json.loads(out.read_text())
    same = True
    for rec, ids in zip(res["prompts"], world["ids"]):
        assert rec["prompt_tokens"] == 64 and len(rec["new_ids"]) == 4
        assert rec["new_ids"] == generate.greedy(grouped, ids.cuda(), 4)[0, 64:].tolist()  # the command line is the API
        same = same and rec["new_ids"] == generate.greedy(world["packed"], ids.cuda(), 4)[0, 64:].tolist()
    if not same:
        # a near-tie of two logits may flip an argmax between two correct forwards: then the logits themselves are held to
        # test_gpu_moe_model.py's criterion instead, teacher-forced -- max |grouped - fp32| <= 2 floor, floor the dense fp16 model's
        ids = world["ids"][0].cuda()
        with torch.no_grad():
            ref = world["fp32"](ids).logits[:, N_PROMPT:]
        floor = float((incremental(world["dense"], ids) - ref).abs().max())
        err = float((incremental(grouped, ids) - ref).abs().max())
        print(f"greedy tokens differ between the two prefill paths; teacher-forced: floor {floor!r}, grouped against fp32 {err!r}")
        assert floor > 0 and err <= 2 * floor
