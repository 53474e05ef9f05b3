"""The packed MoE decode step on int8 activations (K38): gq_gemv_packed_experts_a8 per named pair against fp64 on
tests/act_q8_spec.py's quantized activations (test_gpu_qgemm_a8.py's derived bound, which holds for any summation order) and
bit for bit against gq_gemv_packed_a8 on the expert's slice, the second turn of its grid-stride loop, SwiGLU fused into the
prologue, and PackedExperts(decode_act="q8") against the composition of its ops."""
import numpy as np
import pytest

import act_q8_spec as spec
from test_gpu_qgemm import BF16, F16, FILL, Q4, Q6, Q8, TYPES, bits, guarded_y, guards_intact, ops, packed_weight  # noqa: F401
from test_gpu_qgemm_a8 import OFFSET, activations, bound2

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

IQ4_XS = 23
E = 5
# eight pairs: expert 3 named by five (a second pass of one), expert 0 by one, experts 1, 2, 4 unhit, one id of -1, one of E
IDS = [3, 0, 3, -1, 3, E, 3, 3]
# R = 1, a partial last row group (130) and a partial only group after two whole ones (35); C = 4352: 17 superblocks, a wave's
# partial second step; pairs_per_row 2 (x_rows 4) and 1.  C = 256 has one term per output, which in fp16 can be a subnormal
# without the relative rounding the bound assumes (test_gpu_qgemv_a8.py): those cases run in bf16, the others in fp16.
GRID = [(R, C, ppr) for R in (1, 130, 35) for ppr in (2, 1) for C in (256, 4352)]
CASES = [(R, C, ppr, TYPES[(i + i // 6) % 6], BF16 if C == 256 else F16) for i, (R, C, ppr) in enumerate(GRID)]  # every type in both


def stacked(ops, t, n, R, C, seed):  # noqa: F811
    """[n, R, C] packed; the 2-byte aligned types at byte +2 of their buffer."""
    return packed_weight(ops, t, n * R, C, seed=seed, scale=0.02, offset=OFFSET.get(t, 0))[0]


def call(ops, t, src, n, R, x, ids, ppr, x_up=None):  # noqa: F811
    """One raw call into a FILL-ed, guarded y -> y; the binding must repeat the written rows."""
    from gptq_gguf_toolkit_amd import _cabi
    from gptq_gguf_toolkit_amd.ops import _DT, _ptr, _stream
    pe = torch.tensor(ids, dtype=torch.int32, device="cuda")
    buf, y = guarded_y(len(ids), R, x.dtype)
    _cabi.check(_cabi.lib().gq_gemv_packed_experts_a8(t, _ptr(src), n, R, x.shape[1], _ptr(x), _ptr(x_up), x.shape[0], _ptr(pe),
                                                      len(ids), ppr, _DT[x.dtype], _ptr(y), _stream(x)), "gq_gemv_packed_experts_a8")
    assert guards_intact(buf), "written outside [y, y + P * R * 2)"
    named = [p for p, e in enumerate(ids) if 0 <= e < n]
    skipped = [p for p in range(len(ids)) if p not in named]
    assert bool((bits(y[skipped]) == FILL).all()), "the row of a pair that names no expert was written"
    assert torch.equal(bits(ops.gemv_packed_experts_q8(t, src, n, R, x, pe, ppr, x_up)[named]), bits(y[named]))
    return y, named


# ------------------------------------------------------------------------------------------------ 1, 2: fp64 and bit for bit
@pytest.mark.parametrize("R,C,ppr,t,dt", CASES, ids=[f"R{c[0]}-C{c[1]}-ppr{c[2]}-q{c[3]}-{str(c[4])[6:]}" for c in CASES])
def test_named_pairs_against_fp64_and_gemv_packed_q8_on_the_slice(ops, R, C, ppr, t, dt):  # noqa: F811
    src = stacked(ops, t, E, R, C, seed=3800 + t + R + C)
    x, xf = activations(len(IDS) // ppr, C, dt, seed=R + C + ppr)
    if C > 256:
        x[-1, 512:768] = 0                          # an all-zero superblock: d = 0, codes 0
        x[0, 300] = -x[0, 256:512].abs().max() * 2  # a superblock whose maximum is negative
        xf = x.float().cpu().numpy()
    y, named = call(ops, t, src, E, R, x, IDS, ppr)
    q = spec.quantize(xf)
    for p in named:
        e, row = IDS[p], p // ppr
        ref, mag = spec.terms(t, src.view(E, R, -1)[e].cpu().numpy(), *(a[row:row + 1] for a in q))
        err, bound = np.abs(y[p:p + 1].double().cpu().numpy() - ref), bound2(t, ref, mag, C, dt)
        print(f"pair {p} expert {e}: max err / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (p, float((err / bound).max()))
        assert torch.equal(bits(ops.gemv_packed_q8(t, src.view(E, -1)[e], x[row:row + 1])), bits(y[p:p + 1])), p


# ------------------------------------------------------------------------------------------------ 3: the second turn
@pytest.mark.parametrize("t", [Q4, Q6], ids=["q4k-16-byte", "q6k-2-byte"])
def test_rows_of_a_second_turn_equal_the_same_rows_called_alone(ops, t):  # noqa: F811
    C, dt, ids = 256, BF16, [1, 0, 1]
    plan = ops.gemv_experts_a8_plan(len(ids), 1, C)
    first = plan["grid_x_cap"] * plan["rows_per_turn"]  # an expert's rows of the first turn of a full grid
    R = first + plan["rows_per_turn"] + 5               # workgroup 0 takes a whole second turn, workgroup 1 five rows of one
    assert ops.gemv_experts_a8_plan(len(ids), R, C)["grid_x"] == plan["grid_x_cap"] and plan["fits"]
    src = stacked(ops, t, 2, R, C, seed=5100 + t)
    x, _ = activations(len(ids), C, dt, seed=11)
    y, _ = call(ops, t, src, 2, R, x, ids, 1)
    lo = first - 3
    for p, e in enumerate(ids):
        alone = ops.gemv_packed_q8(t, src.view(2, R, -1)[e, lo:], x[p:p + 1])  # the same rows as turn 0 of another grid
        assert torch.equal(bits(alone), bits(y[p:p + 1, lo:])), p


# ------------------------------------------------------------------------------------------------ 4: SwiGLU in the prologue
@pytest.mark.parametrize("t,dt", [(Q4, F16), (Q8, BF16)], ids=["q4k-f16", "q8_0-bf16"])
def test_fused_swiglu_is_the_same_call_on_fwd_silu_mul(ops, t, dt):  # noqa: F811
    n, R, C, ids = 3, 18, 768, [1, 0, 1, 1, 0]
    src = stacked(ops, t, n, R, C, seed=5200 + t)
    gate, up = activations(len(ids), C, dt, seed=12)[0] * 3, activations(len(ids), C, dt, seed=13)[0]
    up[-1, 512:768] = 0                     # an all-zero superblock: d = 0, codes 0
    gate[0, 300], up[0, 300] = 30.0, -60.0  # a superblock whose maximum is negative
    fused, named = call(ops, t, src, n, R, gate, ids, 1, x_up=up)
    plain, _ = call(ops, t, src, n, R, ops.fwd_silu_mul(gate, up), ids, 1)
    assert named == list(range(len(ids))) and torch.equal(bits(fused), bits(plain))
    assert bool(torch.isfinite(fused).all()) and float(fused.float().abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 5: the module
def test_packed_experts_decode_act_q8_is_the_composition_of_its_ops(ops):  # noqa: F811
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts
    n, H, I, K, dt = 5, 256, 512, 2, F16  # the tiny MoE's expert shape
    shape = {"gate": (I, H), "up": (I, H), "down": (H, I)}
    types = {"gate": Q4, "up": Q6, "down": Q8}
    lv = {r: packed_weight(ops, t, n * shape[r][0], shape[r][1], seed=60 + t, scale=0.05)[0] for r, t in types.items()}
    fp, q8 = PackedExperts(n, H, I, dt), PackedExperts(n, H, I, dt)
    for m in (fp, q8):
        for r in lv:
            m.set_level(r, lv[r], types[r])
    q8.decode_act = "q8"
    assert PackedExperts.decode_act == "fp" and fp.decode_act == "fp"
    g = torch.Generator().manual_seed(5)
    x5 = activations(5, H, dt, seed=14)[0]
    idx5 = torch.stack([torch.randperm(n - 1, generator=g)[:K] for _ in range(5)]).cuda()  # the last expert: never routed to
    w5 = torch.softmax(torch.randn(5, K, generator=g), -1).to(dt).cuda()
    for T in (1, 4):
        x, idx, w = x5[:T], idx5[:T], w5[:T]
        assert q8.takes_q8_decode_path(T, K) and not fp.takes_q8_decode_path(T, K)
        ids = idx.reshape(-1).tolist()

        def per_pair(role, inp, ppr):
            return torch.cat([ops.gemv_packed_q8(types[role], lv[role].view(n, -1)[e], inp[p // ppr:p // ppr + 1])
                              for p, e in enumerate(ids)])

        down = per_pair("down", ops.fwd_silu_mul(per_pair("gate", x, K), per_pair("up", x, K)), 1)
        out = q8(x, idx, w)
        assert torch.equal(bits(out), bits(q8._combine(down, idx.reshape(-1).to(torch.int32), w)))
        base = fp(x, idx, w)
        assert bool(torch.isfinite(out).all()) and not torch.equal(bits(out), bits(base))
        pairs = idx.reshape(-1).to(torch.int32)  # the default module: K24's launches, unchanged
        h = ops.fwd_silu_mul(ops.gemv_packed_experts(Q4, lv["gate"], n, I, x, pairs, K), ops.gemv_packed_experts(Q6, lv["up"], n, I, x, pairs, K))
        assert torch.equal(bits(base), bits(fp._combine(ops.gemv_packed_experts(Q8, lv["down"], n, H, h, pairs, 1), pairs, w)))
    assert not q8.takes_q8_decode_path(5, K)
    assert torch.equal(bits(q8(x5, idx5, w5)), bits(fp(x5, idx5, w5)))  # T = 5: the 16-bit launches
    iq = ops.quantize_iq4(torch.randn(n * I, H, generator=g).cuda() * 0.05, IQ4_XS).view(-1)
    for m in (fp, q8):
        m.set_level("up", iq, IQ4_XS)
    assert not q8.takes_q8_decode_path(1, K)
    assert torch.equal(bits(q8(x5[:1], idx5[:1], w5[:1])), bits(fp(x5[:1], idx5[:1], w5[:1])))  # a role outside A8_TYPES
