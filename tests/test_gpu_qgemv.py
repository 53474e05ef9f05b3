"""The packed-weight decode on the GPU: gq_gemv_packed (K22) against the block decoder (bit for bit), against fp64, against
itself (determinism) and against the tile kernel gq_linear_packed, plus its binding's refusals.  Weights, guards and the
identity cases are test_gpu_qgemm.py's."""
import pytest

from test_gpu_decode import bits
from test_gpu_qgemm import (BF16, F16, IDENTITY, Q3, Q4, Q5, Q8, TYPES, guarded_y, guards_intact, ops,  # noqa: F401
                            packed_weight, subnormal)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def raw_call(t, src, rows, R, C, x, T, y):
    from gptq_gguf_toolkit_amd import _cabi
    from gptq_gguf_toolkit_amd.ops import _DT, _ptr, _stream
    _cabi.check(_cabi.lib().gq_gemv_packed(t, _ptr(src), _ptr(rows), R, C, _ptr(x), T, _DT[x.dtype], _ptr(y), _stream(x)),
                "gq_gemv_packed")


# ------------------------------------------------------------------------------------------------ 1: x = I gives the decoder
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("t,R,C,off,gather", IDENTITY, ids=[f"q{c[0]}-{c[1]}x{c[2]}" for c in IDENTITY])
def test_identity_activations_reproduce_the_decoder(ops, t, R, C, off, gather, dt):  # noqa: F811
    """Sixteen rows of the identity per call (T = 16): the C / 16 results, concatenated, are the decoded weight transposed."""
    src, rows = packed_weight(ops, t, R, C, seed=1000 + t + R, offset=off, gather=gather)
    want = ops.dequantize_blocks(t, src.view(R, -1), dt, rows)
    eye = torch.eye(C, dtype=dt, device="cuda")
    y = torch.cat([ops.gemv_packed(t, src, eye[g:g + 16], rows) for g in range(0, C, 16)])
    assert y.shape == (C, R) and y.dtype == dt
    sub = subnormal(want)  # the guides do not say whether the matrix pipe keeps 16-bit subnormal operands: left out
    n_sub = int(sub.sum())
    print(f"q_type {t} {dt}: {n_sub} subnormal expected values of {want.numel()}, "
          f"{int((y.T[sub] != want[sub]).sum())} of them differ")
    assert n_sub <= 0.01 * want.numel()
    assert bool(torch.isfinite(want).all())
    assert torch.equal(y.T[~sub], want[~sub]), f"{int((y.T != want)[~sub].sum())} of {want.numel()} values differ"


def test_one_hot_rows_reproduce_the_decoder_at_one_token(ops):  # noqa: F811
    t, R, C, off, gather = IDENTITY[1]  # Q3_K [5, 768] at +2 bytes
    src, rows = packed_weight(ops, t, R, C, seed=1000 + t + R, offset=off, gather=gather)
    want = ops.dequantize_blocks(t, src.view(R, -1), F16, rows)
    eye = torch.eye(C, dtype=F16, device="cuda")
    for c in (0, 15, 16, 255, 256, 511, 767):  # first and last column of a lane, of a chunk, of a superblock, of the row
        y = ops.gemv_packed(t, src, eye[c:c + 1], rows)
        assert y.shape == (1, R) and not bool(subnormal(want[:, c]).any())
        assert torch.equal(y[0], want[:, c]), c


# ------------------------------------------------------------------------------------------------ 2: random x against fp64
# C = 2816: 11 superblocks, uneven over any number of waves; C = 256: one superblock, fewer than waves.  R = 130: nine
# workgroups, the last one cut to two rows (2-byte stores: 130 % 4 != 0); R = 1: one row.  The extra case: 65 workgroups, the
# last cut to six rows, two superblocks.
GRID = [(T, R, C) for T in (1, 2, 7, 16) for R in (1, 130) for C in (256, 2816)] + [(3, 1030, 512)]
CASES = [(T, R, C, TYPES[i % 6], (F16, BF16)[(i + i // 6) % 2]) for i, (T, R, C) in enumerate(GRID)]  # every type in both dtypes
IDS = [f"T{c[0]}-R{c[1]}-C{c[2]}-q{c[3]}-{str(c[4])[6:]}" for c in CASES]
_case_cache = {}


def case(ops, T, R, C, t, dt):  # noqa: F811
    """Inputs, the GEMV's result (in guarded memory), fp64 and the bound of one case: computed once, shared by tests 2 and 4.
    bound = u |y64| + C 2^-23 (|x| |Wd|^T) + 2^-25 per element, test_gpu_qgemm.py's: the final rounding (u = 2^-11 fp16, 2^-8
    bf16) plus the worst-case fp32 accumulation of C terms in any order.  Derived, not measured."""
    key = (T, R, C, t, dt)
    if key not in _case_cache:
        src, rows = packed_weight(ops, t, R, C, seed=2000 + t + R + C, scale=0.02, gather=(R > 1 and t in (Q3, Q8)))
        x = torch.randn(T, C, generator=torch.Generator().manual_seed(T + C)).to(dt).cuda()
        Wd = ops.dequantize_blocks(t, src.view(R, -1), dt, rows)
        buf, y = guarded_y(T, R, dt)
        raw_call(t, src, rows, R, C, x, T, y)
        y64 = x.double() @ Wd.double().T
        u = 2.0 ** -11 if dt == F16 else 2.0 ** -8
        bound = u * y64.abs() + C * 2.0 ** -23 * (x.double().abs() @ Wd.double().abs().T) + 2.0 ** -25
        _case_cache[key] = dict(src=src, rows=rows, x=x, buf=buf, y=y, y64=y64, bound=bound)
    return _case_cache[key]


@pytest.mark.parametrize("T,R,C,t,dt", CASES, ids=IDS)
def test_random_activations_against_fp64(ops, T, R, C, t, dt):  # noqa: F811
    c = case(ops, T, R, C, t, dt)
    err = (c["y"].double() - c["y64"]).abs()
    worst = float((err / c["bound"]).max())
    print(f"T={T} R={R} C={C} q_type {t} {dt}: max err / bound = {worst:.3f}")
    assert guards_intact(c["buf"]), "written outside [y, y + T * R * 2)"
    assert bool(torch.isfinite(c["y"]).all()) and float(c["y"].float().abs().max()) > 0
    assert bool((err <= c["bound"]).all()), f"max err / bound = {worst}"


# ------------------------------------------------------------------------------------------------ 3: determinism
def test_the_same_call_gives_the_same_bits(ops):  # noqa: F811
    T, R, C = 7, 130, 2816
    src, _ = packed_weight(ops, Q4, R, C, seed=3000, scale=0.02)
    x = torch.randn(T, C, generator=torch.Generator().manual_seed(3)).half().cuda()
    a, b = ops.gemv_packed(Q4, src, x), ops.gemv_packed(Q4, src, x)
    assert torch.equal(bits(a), bits(b)) and bool(torch.isfinite(a).all()) and float(a.float().abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 4: the tile kernel
@pytest.mark.parametrize("T,R,C,t,dt", CASES, ids=IDS)
def test_agrees_with_the_tile_kernel(ops, T, R, C, t, dt):  # noqa: F811
    """Both kernels lie within `bound` of the same fp64 value, so within 2 bound of each other."""
    c = case(ops, T, R, C, t, dt)
    tile = ops.linear_packed(t, c["src"], c["x"], c["rows"])
    diff = (c["y"].double() - tile.double()).abs()
    print(f"T={T} R={R} C={C} q_type {t} {dt}: max |gemv - linear_packed| / bound = {float((diff / c['bound']).max()):.3f}, "
          f"{int((bits(c['y']) != bits(tile)).sum())} of {tile.numel()} results differ in bits")
    assert bool((diff <= 2 * c["bound"]).all())


# ------------------------------------------------------------------------------------------------ 5: the binding's refusals
def test_gemv_packed_binding_refusals(ops):  # noqa: F811
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
                       ((Q4, src, torch.zeros(3, 128, dtype=F16, device="cuda")), "C=128"),
                       ((Q4, src, torch.zeros(0, 256, dtype=F16, device="cuda")), "non-empty"),  # an empty x
                       ((Q4, src, torch.zeros(17, 256, dtype=F16, device="cuda")), r"T=17.*16.*linear_packed")):
        with pytest.raises(_cabi.GQError, match=word):
            ops.gemv_packed(*args)
    if torch.cuda.device_count() > 1:
        with pytest.raises(_cabi.GQError, match="one device"):
            ops.gemv_packed(Q4, src, x.to("cuda:1"))
    assert ops.gemv_packed(Q4, src, x.view(1, 3, 256)).shape == (1, 3, 4)                     # any leading shape
    assert ops.gemv_packed(Q4, src, torch.zeros(2, 8, 256, dtype=F16, device="cuda")).shape == (2, 8, 4)
    y16 = torch.empty(16, 4, dtype=F16, device="cuda")  # T = 16 with good arguments passes every host check and launches
    raw_call(Q4, src, None, 4, 256, torch.zeros(16, 256, dtype=F16, device="cuda"), 16, y16)
    assert bool((y16 == 0).all())
    with pytest.raises(_cabi.GQError, match="T=17"):  # the library's own refusal, behind the binding's
        raw_call(Q4, src, None, 4, 256, torch.zeros(17, 256, dtype=F16, device="cuda"), 17, torch.empty(17, 4, dtype=F16, device="cuda"))
