"""The packed MoE prefill on int8 activations (K36) on the GPU: gq_linear_packed_experts_a8 against gq_linear_packed_a8 on the
expert's slice (bit for bit: the header's contract) and against fp64 on the same quantized activations (test_gpu_qgemm_a8.py's
derived bound), gq_silu_mul_quantize_act_q8 byte for byte against the two launches it replaces, and PackedExperts(act="q8")
against the composition of its ops.  Shapes are test_gpu_moe_prefill.py's: E = 3 with expert 2 never named, R = 40 and 130,
C = 512."""
import pytest

import act_q8_spec as spec
from test_gpu_decode import bits
from test_gpu_moe_gemv import inputs, stacked
from test_gpu_moe_prefill import ROWS, C, E, pair_sets
from test_gpu_qgemm import BF16, F16, FILL, Q4, Q6, Q8, TYPES, guarded_y, guards_intact, ops, packed_weight  # noqa: F401
from test_gpu_qgemm_a8 import bound2, on_device

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

IQ4_XS = 23


def all_pair_sets():
    """test_gpu_moe_prefill.py's, and runs of 33 and 31 pairs: a second 32-token sub-tile that holds one token, and a run one
    short of a sub-tile."""
    g = torch.Generator().manual_seed(36)
    ids = [0] * 33 + [1] * 31
    return dict(pair_sets(), **{"33-and-31": (64, 1, [ids[i] for i in torch.randperm(64, generator=g).tolist()])})


def raw_call(t, src, R, q, ppr, route, y):
    from gptq_gguf_toolkit_amd import _cabi
    from gptq_gguf_toolkit_amd.ops import _DT, _ptr, _stream
    xq, xd, xbsum = q
    return _cabi.lib().gq_linear_packed_experts_a8(t, _ptr(src), E, R, C, _ptr(xq), _ptr(xd), _ptr(xbsum), xq.shape[0], ppr,
                                                   _ptr(route[0]), _ptr(route[1]), route[1].numel(), _ptr(y), _DT[y.dtype],
                                                   _stream(xq))


def pairs_of(ids, e):
    return [p for p, v in enumerate(ids) if v == e]


# ------------------------------------------------------------------------------------------------ 1: the contract
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("t", TYPES, ids=[f"q{t}" for t in TYPES])
def test_every_pair_is_linear_packed_a8_on_its_experts_slice(ops, t, dt):  # noqa: F811
    for R in ROWS:
        src = stacked(ops, t, R, C)
        for name, (x_rows, ppr, ids) in all_pair_sets().items():
            q = ops.quantize_act_q8(inputs(x_rows, C, F16))
            route = ops.moe_route(torch.tensor(ids, dtype=torch.int32, device="cuda"), E)
            buf, y = guarded_y(len(ids), R, dt)
            assert raw_call(t, src, R, q, ppr, route, y) == 0
            assert 2 not in ids
            written = []
            for e in (0, 1):
                mine = pairs_of(ids, e)
                rows = torch.tensor([p // ppr for p in mine], device="cuda")
                want = ops.linear_packed_a8(t, src.view(E, -1)[e], *(a[rows].contiguous() for a in q), out_dtype=dt)
                assert torch.equal(bits(y[mine]), bits(want)), (name, R, e, int((bits(y[mine]) != bits(want)).sum()))
                written += mine
            skipped = sorted(set(range(len(ids))) - set(written))
            assert bool((bits(y[skipped]) == FILL).all()), (name, R, "a skipped pair's row was written")
            assert guards_intact(buf), (name, R, "written outside [y, y + P * R * 2)")
            assert bool(torch.isfinite(y[written]).all()) and float(y[written].float().abs().max()) > 0
            got = ops.linear_packed_experts_a8(t, src, E, R, *q, route, ppr, dt)  # the binding, and the same call again
            assert torch.equal(bits(got[written]), bits(y[written])), (name, R, "two calls differ")


# ------------------------------------------------------------------------------------------------ 2: fp64
@pytest.mark.parametrize("t,dt", [(Q4, F16), (Q6, BF16), (Q8, F16)], ids=["q4k-mins", "q6k-groups-of-16", "q8_0"])
def test_against_fp64_on_the_same_quantized_activations(ops, t, dt):  # noqa: F811
    """test_gpu_qgemm_a8.py's bound2, derived from the header's roundings, per pair against act_q8_spec.terms."""
    R = 130
    x_rows, ppr, ids = pair_sets()["128-and-129"]
    src = stacked(ops, t, R, C)
    q = spec.quantize(inputs(x_rows, C, F16).float().cpu().numpy())
    route = ops.moe_route(torch.tensor(ids, dtype=torch.int32, device="cuda"), E)
    y = ops.linear_packed_experts_a8(t, src, E, R, *on_device(*q), route, ppr, dt).double().cpu().numpy()
    for e in (0, 1):
        mine = pairs_of(ids, e)
        rows = [p // ppr for p in mine]
        ref, mag = spec.terms(t, src.view(E, R, -1)[e].cpu().numpy(), *(a[rows] for a in q))
        err, bound = abs(y[mine] - ref), bound2(t, ref, mag, C, dt)
        worst = float((err / bound).max())
        print(f"q_type {t} {dt} expert {e}: max err / bound = {worst:.3f}")
        assert bool((err <= bound).all()), f"max err / bound = {worst}"


# ------------------------------------------------------------------------------------------------ 3: the fused quantizer
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("P,I", [(1, 256), (5, 768)])
def test_fused_quantizer_is_the_two_launches_byte_for_byte(ops, P, I, dt):  # noqa: F811
    gate, up = inputs(P, I, dt) * 3, inputs(P + 1, I, dt)[1:].contiguous()
    if I > 256:
        up[P - 1, 512:768] = 0                  # an all-zero superblock: d = 0, codes 0
        gate[0, 300], up[0, 300] = 30.0, -60.0  # a superblock whose maximum is negative
        gate[2] = float("nan")                  # what a masked pair's garbage looks like
        up[3, 7] = float("inf")
    h = ops.fwd_silu_mul(gate, up)
    want, got = ops.quantize_act_q8(h), ops.silu_mul_quantize_act_q8(gate, up)
    for name, a, b in zip(("xq", "xd", "xbsum"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
    if I > 256:
        assert float(want[1][P - 1, 2]) == 0 and int(got[0][0, 300]) == -127 and not bool(got[0][2].any())
    assert bool(got[0].any())


# ------------------------------------------------------------------------------------------------ 4: the module
def test_packed_experts_act_q8_is_the_composition_of_its_ops(ops):  # noqa: F811
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts
    n, H, I, K, T, dt = 5, 256, 512, 2, 40, F16  # the tiny MoE's expert shape
    shape = {"gate": (I, H), "up": (I, H), "down": (H, I)}
    lv = {r: packed_weight(ops, t, n * shape[r][0], shape[r][1], seed=60 + t, scale=0.05)[0]
          for r, t in (("gate", Q4), ("up", Q6), ("down", Q8))}
    types = {"gate": Q4, "up": Q6, "down": Q8}
    fp, q8 = PackedExperts(n, H, I, dt), PackedExperts(n, H, I, dt)
    for m in (fp, q8):
        m.prefill = "grouped"
        for r in lv:
            m.set_level(r, lv[r], types[r])
    q8.act = "q8"
    g = torch.Generator().manual_seed(4)
    x = inputs(T, H, dt)
    idx = torch.stack([torch.randperm(n - 1, generator=g)[:K] for _ in range(T)]).cuda()  # the last expert: never routed to
    w = torch.softmax(torch.randn(T, K, generator=g), -1).to(dt).cuda()
    assert q8.takes_q8_path(T, K) and not fp.takes_q8_path(T, K) and not q8.takes_q8_path(1, K)
    out = q8(x, idx, w)
    pairs = idx.reshape(-1).to(torch.int32)
    route = ops.moe_route(pairs, n)
    xa = ops.quantize_act_q8(x)
    gate = ops.linear_packed_experts_a8(Q4, lv["gate"], n, I, *xa, route, K, dt)
    up = ops.linear_packed_experts_a8(Q6, lv["up"], n, I, *xa, route, K, dt)
    down = ops.linear_packed_experts_a8(Q8, lv["down"], n, H, *ops.silu_mul_quantize_act_q8(gate, up), route, 1, dt)
    assert torch.equal(bits(out), bits(q8._combine(down, pairs, w)))
    base = fp(x, idx, w)
    assert bool(torch.isfinite(out).all()) and not torch.equal(bits(out), bits(base))
    assert torch.equal(bits(q8(x[:1], idx[:1], w[:1])), bits(fp(x[:1], idx[:1], w[:1])))  # a decode step: the GEMV on either
    iq = ops.quantize_iq4(torch.randn(n * I, H, generator=g).cuda() * 0.05, IQ4_XS).view(-1)
    for m in (fp, q8):
        m.set_level("up", iq, IQ4_XS)
    assert not q8.takes_q8_path(T, K) and torch.equal(bits(q8(x, idx, w)), bits(fp(x, idx, w)))  # a role outside A8_TYPES: the fp launches
