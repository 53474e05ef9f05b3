"""The packed MoE prefill on the GPU: gq_moe_route (K25) against torch's stable sort, gq_linear_packed_experts against
gq_linear_packed on the expert's slice (bit for bit: the header's contract), against itself (determinism), against fp64
(test_gpu_qgemm.py's bound) and the refusals of both.  Weights, guards and types are test_gpu_qgemm.py's and
test_gpu_moe_gemv.py's: quantized random-normal matrices, so every decode is finite.

Shapes: E = 3 with expert 2 never named (no workgroup stages its bytes); R = 40 (one row tile, 8-byte stores) and R = 130 (two
row tiles, the second of two rows; 130 % 4 != 0: 2-byte stores); C = 512 (two superblocks: every row is staged twice)."""
import pytest

from test_gpu_decode import bits
from test_gpu_moe_gemv import inputs, stacked
from test_gpu_qgemm import BF16, F16, FILL, Q2, Q3, Q4, Q6, Q8, TYPES, guarded_y, guards_intact, ops  # noqa: F401
from test_moe_prefill_cpu import route_by_sort

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E, C = 3, 512
ROWS = (40, 130)
BAD_TYPE, BAD_SHAPE, NULL = -1, -2, -6
WORD = 0x5A5A5A5A
GUARD = 16  # int32 words before and after a route output


# ------------------------------------------------------------------------------------------------ 1: the route
def guarded_i32(n):
    buf = torch.full((n + 2 * GUARD,), WORD, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def i32_guards_intact(buf):
    return bool((buf[:GUARD] == WORD).all()) and bool((buf[-GUARD:] == WORD).all())


def raw_route(pe, n_experts, es, order, P=None):
    from gptq_gguf_toolkit_amd import _cabi
    from gptq_gguf_toolkit_amd.ops import _ptr, _stream
    return _cabi.lib().gq_moe_route(_ptr(pe), pe.numel() if P is None else P, n_experts, _ptr(es), _ptr(order), _stream(es))


def drawn_ids(P, n_experts, seed):
    """P ids from [-1, E] (E is transformers' masked pair) with one 2**30 among them."""
    ids = torch.randint(-1, n_experts + 1, (P,), generator=torch.Generator().manual_seed(seed)).to(torch.int32)
    if P > 1:
        ids[P // 2] = 2 ** 30
    return ids.cuda()


ROUTES = [(P, n) for P in (1, 7, 64, 1000, 4099) for n in (1, 3, 256)] + [(131072, 8)]  # and the largest call: 128 chunks


@pytest.mark.parametrize("P,n_experts", ROUTES, ids=[f"P{p}-E{n}" for p, n in ROUTES])
def test_route_is_the_stable_sort(ops, P, n_experts):  # noqa: F811
    cases = [drawn_ids(P, n_experts, seed=P + n_experts)]
    if P == 1:
        cases += [torch.tensor([v], dtype=torch.int32, device="cuda") for v in (0, 2 ** 30, -1, n_experts)]
    if P == 1000:
        cases.append(torch.full((P,), n_experts - 1, dtype=torch.int32, device="cuda"))  # every pair on the last expert
    for pe in cases:
        want_start, want_order = route_by_sort(pe, n_experts)
        sbuf, es = guarded_i32(n_experts + 1)
        obuf, order = guarded_i32(P)
        assert raw_route(pe, n_experts, es, order) == 0
        assert torch.equal(es, want_start), (es.tolist()[:8], want_start.tolist()[:8])
        assert torch.equal(order, want_order), int((order != want_order).sum())
        assert i32_guards_intact(sbuf) and i32_guards_intact(obuf), "written outside expert_start[0 .. E] / order[0 .. P)"
        sbuf2, es2 = guarded_i32(n_experts + 1)
        obuf2, order2 = guarded_i32(P)
        assert raw_route(pe, n_experts, es2, order2) == 0
        assert torch.equal(es2, es) and torch.equal(order2, order), "two calls differ"
        a, b = ops.moe_route(pe, n_experts)  # the binding: the same call
        assert torch.equal(a, es) and torch.equal(b, order)


# ------------------------------------------------------------------------------------------------ 2: the contract
def pair_sets():
    """name -> (x_rows, pairs_per_row, expert ids); expert 2 is never named."""
    g = torch.Generator().manual_seed(11)
    t5 = torch.stack([torch.randperm(2, generator=g) for _ in range(5)]).reshape(-1).tolist()  # distinct experts per token
    t301 = [1] * 301
    t301[137] = 0                                                                 # one pair on expert 0 amid 300 on expert 1
    c257 = [0] * 128 + [1] * 129
    c257 = [c257[i] for i in torch.randperm(257, generator=g).tolist()]
    return {"T5-K2": (5, 2, t5),
            "T301-K1": (301, 1, t301),                                            # three token tiles of 128 on expert 1
            "128-and-129": (257, 1, c257),                                        # a full tile; a full tile and one pair
            "masked": (4, 2, [0, 1, E, 0, 1, -1, 2 ** 30, 1]),                    # pairs 2, 5 and 6 name no expert
            "P200": (200, 1, torch.randint(0, 2, (200,), generator=g).tolist())}  # pairs_per_row = 1 (the down projection)


def raw_call(t, src, R, x, ppr, route, y, n_experts=E, C=C, P=None, x_dtype=None):
    """-> the status; y is the caller's."""
    from gptq_gguf_toolkit_amd import _cabi
    from gptq_gguf_toolkit_amd.ops import _DT, _ptr, _stream
    es, order = route
    return _cabi.lib().gq_linear_packed_experts(t, _ptr(src), n_experts, R, C, _ptr(x), x.shape[0], ppr, _ptr(es), _ptr(order),
                                                order.numel() if P is None else P, _DT[x.dtype] if x_dtype is None else x_dtype,
                                                _ptr(y), _stream(x))


def expected_rows(ops, t, src, ids, x, ppr, n_experts=E):  # noqa: F811
    """{pair: its row of ops.linear_packed(t, slice of its expert, the x rows of that expert's pairs)}: the per-expert GEMM
    the loop path runs, with all of the expert's tokens in one call."""
    slices = src.view(n_experts, -1)
    want = {}
    for e in sorted({e for e in ids if 0 <= e < n_experts}):
        mine = [p for p, v in enumerate(ids) if v == e]
        rows = torch.tensor([p // ppr for p in mine], device="cuda")
        y = ops.linear_packed(t, slices[e], x[rows].contiguous())
        want.update({p: y[i] for i, p in enumerate(mine)})
    return want


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("t", TYPES, ids=[f"q{t}" for t in TYPES])
def test_every_pair_is_linear_packed_on_its_experts_slice(ops, t, dt):  # noqa: F811
    """Every written row == the row of linear_packed on that expert's slice and gathered tokens, with torch.equal on the
    bits, and for a few rows also == the T = 1 call of the header's contract; a second call gives the same bits; nothing
    outside y is written and a masked pair's row keeps the fill."""
    for R in ROWS:
        src = stacked(ops, t, R, C)
        slices = src.view(E, -1)
        for name, (x_rows, ppr, ids) in pair_sets().items():
            x = inputs(x_rows, C, dt)
            pe = torch.tensor(ids, dtype=torch.int32, device="cuda")
            route = ops.moe_route(pe, E)
            buf, y = guarded_y(len(ids), R, dt)
            assert raw_call(t, src, R, x, ppr, route, y) == 0
            want = expected_rows(ops, t, src, ids, x, ppr)
            assert 2 not in ids and len(want) == sum(0 <= e < E for e in ids)
            for p, e in enumerate(ids):
                if p not in want:
                    assert bool((bits(y[p]) == FILL).all()), (name, R, p, "a skipped pair's row was written")
                else:
                    assert torch.equal(bits(y[p]), bits(want[p])), (name, R, p, e, int((bits(y[p]) != bits(want[p])).sum()))
            for p in sorted(want)[::max(1, len(want) // 3)]:  # the contract as the header words it: the T = 1 call
                one = ops.linear_packed(t, slices[ids[p]], x[p // ppr:p // ppr + 1])[0]
                assert torch.equal(bits(y[p]), bits(one)), (name, R, p, "differs from the T = 1 call")
            assert guards_intact(buf), (name, R, "written outside [y, y + P * R * 2)")
            written = y[sorted(want)]
            assert bool(torch.isfinite(written).all()) and float(written.float().abs().max()) > 0
            buf2, y2 = guarded_y(len(ids), R, dt)
            assert raw_call(t, src, R, x, ppr, route, y2) == 0
            assert torch.equal(bits(y2), bits(y)), (name, R, "two calls differ")
            got = ops.linear_packed_experts(t, src, E, R, x, route, ppr)  # the binding: the same call
            assert torch.equal(bits(got[sorted(want)]), bits(written)), (name, R)


WIDE = [(Q2, F16), (Q3, BF16), (Q6, F16), (Q8, BF16), (Q4, BF16)]


@pytest.mark.parametrize("t,dt", WIDE, ids=[f"q{t}" for t, _ in WIDE])
def test_the_wide_token_tile_gives_the_same_bits(ops, t, dt):  # noqa: F811
    """P = 1280 >= 128 E pairs: the smallest kind of call that takes the 256-token tile (Q4_K keeps the 128-token one at any
    size), with some 420 pairs on each of two experts: two tiles of 256 each, the second cut.  The reference, linear_packed
    with one expert's tokens, runs its 128-token tile here: equal bits across the two widths and the two kernels.  Ids from
    [-1, E) without expert 2; both row-tile shapes."""
    ppr, x_rows = 8, 160
    g = torch.Generator().manual_seed(t)
    ids = torch.randint(-1, 2, (x_rows * ppr,), generator=g)
    pe = ids.to(torch.int32).cuda()
    assert pe.numel() >= 128 * E
    x = inputs(x_rows, C, dt)
    route = ops.moe_route(pe, E)
    for R in ROWS:
        src = stacked(ops, t, R, C)
        buf, y = guarded_y(x_rows * ppr, R, dt)
        assert raw_call(t, src, R, x, ppr, route, y) == 0
        for e in (0, 1):
            mine = (pe == e).nonzero().view(-1)
            want = ops.linear_packed(t, src.view(E, -1)[e], x[mine // ppr].contiguous())
            assert mine.numel() > 256 and torch.equal(bits(y[mine]), bits(want)), (R, e, int((bits(y[mine]) != bits(want)).sum()))
        assert bool((bits(y[(pe < 0).nonzero().view(-1)]) == FILL).all()) and guards_intact(buf), R


# ------------------------------------------------------------------------------------------------ 3: fp64
@pytest.mark.parametrize("i,t", list(enumerate(TYPES)), ids=[f"q{t}" for t in TYPES])
def test_against_fp64(ops, i, t):  # noqa: F811
    """test_gpu_qgemm.py's bound: u |y64| + C 2^-23 (|x| |Wd|^T) + 2^-25 per element, u = 2^-11 fp16 / 2^-8 bf16 -- the
    final rounding plus the worst-case fp32 accumulation of C terms in any order.  One configuration per type: [130, 512],
    the 200 pairs of "P200", the dtypes alternating."""
    R, dt = 130, (F16, BF16)[i % 2]
    x_rows, ppr, ids = pair_sets()["P200"]
    src = stacked(ops, t, R, C)
    x = inputs(x_rows, C, dt)
    pe = torch.tensor(ids, dtype=torch.int32, device="cuda")
    y = ops.linear_packed_experts(t, src, E, R, x, ops.moe_route(pe, E), ppr)
    Wd = ops.dequantize_blocks(t, src.view(E * R, -1), dt).view(E, R, C).double()
    xp = x.double()[torch.arange(len(ids), device="cuda") // ppr]
    Wp = Wd[pe.long()]
    y64 = torch.einsum("prc,pc->pr", Wp, xp)
    u = 2.0 ** -11 if dt == F16 else 2.0 ** -8
    bound = u * y64.abs() + C * 2.0 ** -23 * torch.einsum("prc,pc->pr", Wp.abs(), xp.abs()) + 2.0 ** -25
    err = (y.double() - y64).abs()
    worst = float((err / bound).max())
    print(f"q_type {t} {dt}: max err / bound = {worst:.3f}")
    assert bool(torch.isfinite(y).all()) and float(y.float().abs().max()) > 0
    assert bool((err <= bound).all()), f"max err / bound = {worst}"


# ------------------------------------------------------------------------------------------------ 4: refusals
def test_refusals_return_the_status_and_launch_nothing(ops):  # noqa: F811
    from gptq_gguf_toolkit_amd import _cabi
    R = 40
    src = stacked(ops, Q4, R, C)
    x = inputs(2, C, F16)
    pe = torch.tensor([0, 1, 1, 0], dtype=torch.int32, device="cuda")
    route = ops.moe_route(pe, E)
    buf, y = guarded_y(4, R, F16)
    L = _cabi.lib()
    for status, word, kw in ((BAD_TYPE, "q_type 9", dict(t=9)),
                             (BAD_TYPE, "x_dtype 0", dict(x_dtype=0)),  # (0 is the library's code of fp32)
                             (NULL, "order is NULL", dict(route=(route[0], None), P=4)),
                             (BAD_SHAPE, "E=0", dict(n_experts=0)),
                             (BAD_SHAPE, "E=257", dict(n_experts=257)),
                             (BAD_SHAPE, "R=0", dict(R=0)),
                             (BAD_SHAPE, "P=131073", dict(P=131073)),
                             (BAD_SHAPE, "x_rows=2 * pairs_per_row=1 != P=4", dict(ppr=1)),
                             (BAD_SHAPE, "C=128", dict(C=128)),
                             (BAD_SHAPE, "blocks not 16-byte aligned", dict(src=src[8:])),
                             (BAD_SHAPE, "order not 4-byte aligned", dict(route=(route[0], route[1].view(torch.int16)[1:]), P=4)),
                             (BAD_SHAPE, "x not 16-byte aligned", dict(x=inputs(3, C, F16).view(-1)[4:4 + 2 * C].view(2, C)))):
        args = dict(t=Q4, src=src, R=R, x=x, ppr=2, route=route, y=y)
        args.update(kw)
        rc = raw_call(**args)
        assert rc == status and word in L.gq_last_error().decode(), (kw, rc, L.gq_last_error().decode())
    sbuf, es = guarded_i32(E + 1)
    obuf, order = guarded_i32(4)
    for status, word, a in ((NULL, "pair_expert is NULL", (None, E, es, order, 4)),
                            (BAD_SHAPE, "E=0", (pe, 0, es, order)),
                            (BAD_SHAPE, "E=257", (pe, 257, es, order)),
                            (BAD_SHAPE, "order not 4-byte aligned", (pe, E, es, order.view(torch.int16)[1:]))):
        assert raw_route(*a) == status and word in L.gq_last_error().decode(), (word, L.gq_last_error().decode())
    torch.cuda.synchronize()
    assert bool((bits(buf) == FILL).all()), "a refused call wrote to y"
    assert bool((sbuf == WORD).all()) and bool((obuf == WORD).all()), "a refused route wrote to its outputs"
    with pytest.raises(_cabi.GQError, match="one device|CPU"):
        ops.linear_packed_experts(Q4, src, E, R, x, (route[0].cpu(), route[1]), 2)
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.moe_route(pe.cpu(), E)
    assert raw_call(Q4, src, R, x, 2, route, y) == 0 and float(y.float().abs().max()) > 0  # and the good call launches
