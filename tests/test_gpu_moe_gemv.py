"""The grouped expert GEMV on the GPU: gq_gemv_packed_experts (K24) against gq_gemv_packed on the expert's slice (bit for
bit: the header's contract), against itself (determinism), against fp64 (test_gpu_qgemv.py's bound) and its refusals.
Weights, guards and types are test_gpu_qgemm.py's: quantized random-normal matrices, so every decode is finite.

Shapes: E = 3 with expert 2 never named (its workgroups return before staging); R = 40 (three workgroups, the last one cut to
eight rows, 8-byte stores) and R = 18 (two rows in the last workgroup, 2-byte stores: 18 % 4 != 0); C = 512 (two waves, one
superblock each) and C = 4352 (17 superblocks: wave 0 takes a second one)."""
import pytest

from test_gpu_decode import bits
from test_gpu_qgemm import BF16, F16, FILL, Q4, TYPES, guarded_y, guards_intact, ops, packed_weight  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E = 3
SHAPES = [(40, 512), (18, 512), (40, 4352), (18, 4352)]
BAD_TYPE, BAD_SHAPE, NULL = -1, -2, -6


def pair_sets():
    """name -> (x_rows, pairs_per_row, expert ids); expert 2 is never named."""
    g = torch.Generator().manual_seed(7)
    t16 = torch.stack([torch.randperm(2, generator=g) for _ in range(16)]).reshape(-1).tolist()  # distinct experts per token
    return {"T1-K2": (1, 2, [1, 0]),
            "T16-K2": (16, 2, t16),                       # 32 pairs, 16 per expert: one full pass each
            "P64-one-expert": (64, 1, [1] * 64),          # four passes of 16 in the workgroups of expert 1
            "masked": (3, 2, [0, 1, E, 0, 1, 0])}         # pair 2 names no expert: its row of y stays as it was


def raw_call(t, src, R, C, x, pe, ppr, y, E=E):
    """-> the status; y is the caller's."""
    from gptq_gguf_toolkit_amd import _cabi
    from gptq_gguf_toolkit_amd.ops import _DT, _ptr, _stream
    return _cabi.lib().gq_gemv_packed_experts(t, _ptr(src), E, R, C, _ptr(x), x.shape[0], _ptr(pe), pe.numel(), ppr,
                                              _DT[x.dtype], _ptr(y), _stream(x))


_cache = {}


def stacked(ops, t, R, C):  # noqa: F811
    """The packed [E, R, C] tensor of one type and shape: quantized once, shared by every test."""
    if (t, R, C) not in _cache:
        src, _ = packed_weight(ops, t, E * R, C, seed=5000 + t + R + C, scale=0.02)
        _cache[(t, R, C)] = src
    return _cache[(t, R, C)]


def inputs(x_rows, C, dt):
    return torch.randn(x_rows, C, generator=torch.Generator().manual_seed(x_rows + C)).to(dt).cuda()


# ------------------------------------------------------------------------------------------------ 1, 2: the contract, twice
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("t", TYPES, ids=[f"q{t}" for t in TYPES])
def test_every_pair_is_gemv_packed_on_its_experts_slice(ops, t, dt):  # noqa: F811
    """Row p == gemv_packed(t, slice of expert pair_expert[p], x[p // pairs_per_row]) with torch.equal on the bits, for
    every shape and pair set; a second call gives the same bits; nothing outside y is written and a masked pair's row keeps
    the fill."""
    for R, C in SHAPES:
        src = stacked(ops, t, R, C)
        slices = src.view(E, -1)
        singles = {}
        for name, (x_rows, ppr, ids) in pair_sets().items():
            x = inputs(x_rows, C, dt)
            pe = torch.tensor(ids, dtype=torch.int32, device="cuda")
            buf, y = guarded_y(len(ids), R, dt)
            assert raw_call(t, src, R, C, x, pe, ppr, y) == 0
            for p, e in enumerate(ids):
                row = p // ppr
                if e >= E:
                    assert bool((bits(y[p]) == FILL).all()), (name, R, C, p, "a skipped pair's row was written")
                    continue
                if (name, e, row) not in singles:
                    singles[(name, e, row)] = ops.gemv_packed(t, slices[e], x[row:row + 1])[0]
                want = singles[(name, e, row)]
                assert torch.equal(bits(y[p]), bits(want)), (name, R, C, p, e, int((bits(y[p]) != bits(want)).sum()))
            assert guards_intact(buf), (name, R, C, "written outside [y, y + P * R * 2)")
            written = y[[p for p, e in enumerate(ids) if e < E]]
            assert bool(torch.isfinite(written).all()) and float(written.float().abs().max()) > 0
            buf2, y2 = guarded_y(len(ids), R, dt)
            assert raw_call(t, src, R, C, x, pe, ppr, y2) == 0
            assert torch.equal(bits(y2), bits(y)), (name, R, C, "two calls differ")
            if name != "masked":
                assert torch.equal(bits(ops.gemv_packed_experts(t, src, E, R, x, pe, ppr)), bits(y))  # the binding: the same call


# ------------------------------------------------------------------------------------------------ 3: fp64
@pytest.mark.parametrize("i,t", list(enumerate(TYPES)), ids=[f"q{t}" for t in TYPES])
def test_against_fp64(ops, i, t):  # noqa: F811
    """test_gpu_qgemv.py's bound (its `case`): u |y64| + C 2^-23 (|x| |Wd|^T) + 2^-25 per element, u = 2^-11 fp16 / 2^-8
    bf16 -- the final rounding plus the worst-case fp32 accumulation of C terms in any order.  One configuration per type:
    [40, 4352], sixteen tokens with two experts each, the dtypes alternating."""
    R, C, dt = 40, 4352, (F16, BF16)[i % 2]
    x_rows, ppr, ids = pair_sets()["T16-K2"]
    src = stacked(ops, t, R, C)
    x = inputs(x_rows, C, dt)
    pe = torch.tensor(ids, dtype=torch.int32, device="cuda")
    y = ops.gemv_packed_experts(t, src, E, R, x, pe, ppr)
    Wd = ops.dequantize_blocks(t, src.view(E * R, -1), dt).view(E, R, C).double()
    xp = x.double()[torch.arange(len(ids), device="cuda") // ppr]                      # [P, C]
    Wp = Wd[pe.long()]                                                                  # [P, R, C]
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
    R, C = 40, 512
    src = stacked(ops, Q4, R, C)
    x = inputs(2, C, F16)
    pe = torch.tensor([0, 1, 1, 0], dtype=torch.int32, device="cuda")
    buf, y = guarded_y(4, R, F16)
    L = _cabi.lib()
    for status, word, kw in ((BAD_SHAPE, "P=65", dict(pe=torch.zeros(65, dtype=torch.int32, device="cuda"), x=inputs(65, C, F16), ppr=1)),
                             (BAD_SHAPE, "x_rows=2 * pairs_per_row=1 != P=4", dict(ppr=1)),
                             (BAD_SHAPE, "C=128", dict(C=128)),
                             (BAD_SHAPE, "E=0", dict(E=0)),
                             (BAD_SHAPE, "R=0", dict(R=0)),
                             (BAD_TYPE, "q_type 9", dict(t=9)),
                             (BAD_SHAPE, "blocks not 16-byte aligned", dict(src=src[8:])),
                             (BAD_SHAPE, "x not 16-byte aligned", dict(x=inputs(3, C, F16).view(-1)[4:4 + 2 * C].view(2, C)))):
        args = dict(t=Q4, src=src, R=R, C=C, x=x, pe=pe, ppr=2, y=y)
        args.update(kw)
        assert raw_call(**args) == status and word in L.gq_last_error().decode(), (kw, L.gq_last_error().decode())
    torch.cuda.synchronize()
    assert bool((bits(buf) == FILL).all()), "a refused call wrote to y"
    with pytest.raises(_cabi.GQError, match="one device|CPU"):
        ops.gemv_packed_experts(Q4, src, E, R, x, pe.cpu(), 2)
    with pytest.raises(_cabi.GQError, match="P=65"):
        ops.gemv_packed_experts(Q4, src, E, R, inputs(65, C, F16), torch.zeros(65, dtype=torch.int32, device="cuda"), 1)
    assert raw_call(Q4, src, R, C, x, pe, 2, y) == 0 and float(y.float().abs().max()) > 0  # and the good call launches
