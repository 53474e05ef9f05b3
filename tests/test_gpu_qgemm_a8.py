"""The packed forward on int8 activations (K35): gq_quantize_act_q8 byte for byte against tests/act_q8_spec.py,
gq_linear_packed_a8 against fp64 on the same quantized activations and end to end against fp64 on the unquantized x, and the
opt-in route through PackedLinear and ppleval.  Bounds are derived from the roundings that include/gptq_gguf_qgemm_a8.h
lists, not measured."""
import numpy as np
import pytest

import act_q8_spec as spec
from test_gpu_eval import gguf_model, run_ppleval  # noqa: F401  (gguf_model: the fixture that builds the small .gguf)
from test_gpu_qgemm import BF16, F16, FP64, Q2, Q3, Q4, Q6, Q8, bits, guarded_y, guards_intact, ops, packed_weight  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OFFSET = {Q3: 2, Q6: 2, Q8: 2}  # the 2-byte-aligned types: sources at byte +2 of a 16-byte aligned buffer
U_OUT = {F16: 2.0 ** -11, BF16: 2.0 ** -8}
TINY = 2.0 ** -149


def activations(T, C, dt, seed):
    """x [T, C] in dt (|x| in a normal range) -> (x on the device, its exact values as float32 numpy)."""
    x = torch.randn(T, C, generator=torch.Generator().manual_seed(seed)).to(dt)
    return x.cuda(), x.float().numpy()


def on_device(xq, xd, xbsum):
    return tuple(torch.from_numpy(a).cuda() for a in (xq, xd, xbsum))


def bound2(t, ref, mag, C, dt):
    return U_OUT[dt] * np.abs(ref) + (C // 256 + (12 if t == Q8 else 4)) * 2.0 ** -24 * mag + TINY


# ------------------------------------------------------------------------------------------------ 1: the quantizer
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("T,C", [(1, 256), (5, 256), (1, 768), (5, 768)])
def test_quantizer_is_the_spec_byte_for_byte(ops, T, C, dt):
    x, xf = activations(T, C, dt, seed=T + C)
    if C > 256:
        x[T - 1, 512:768] = 0                       # an all-zero superblock: d = 0, codes 0
        x[0, 300] = -x[0, 256:512].abs().max() * 2  # a superblock whose maximum is negative
        xf = x.float().cpu().numpy()
    xq, xd, xbsum = ops.quantize_act_q8(x)
    wq, wd, wbsum = spec.quantize(xf)
    assert xq.dtype == torch.int8 and xd.dtype == torch.float32 and xbsum.dtype == torch.int16
    assert np.array_equal(xq.cpu().numpy(), wq) and np.array_equal(xbsum.cpu().numpy(), wbsum)
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), wd.view(np.uint32))
    assert np.array_equal(xbsum.cpu().numpy(), xq.cpu().numpy().astype(np.int32).reshape(T, C // 16, 16).sum(axis=2))
    if C > 256:
        assert float(xd[T - 1, 2]) == 0 and not bool(xq[T - 1, 512:768].any()) and int(xq[0, 300]) == -127
        y = ops.linear_packed_q8(Q4, packed_weight(ops, Q4, 3, C, seed=11)[0], x)
        assert bool(torch.isfinite(y).all())  # no NaN downstream of d = 0


# ------------------------------------------------------------------------------------------------ 2: the GEMM against fp64
@pytest.mark.parametrize("T,R,C,t,dt", FP64, ids=[f"T{c[0]}-R{c[1]}-C{c[2]}-q{c[3]}-{str(c[4])[6:]}" for c in FP64])
def test_gemm_against_fp64_on_the_same_quantized_activations(ops, T, R, C, t, dt):
    """|y - ref| <= u_out |ref| + (C/256 + 4) 2^-24 sum_j (|xd d isum_j| + |xd dmin msum_j|) + one fp32 subnormal; Q8_0: the sum
    over its blocks and C/256 + 12 (header: two conversions, three products and a difference per term, one add per superblock;
    Q8_0 a conversion, a product and an add per block)."""
    from gptq_gguf_toolkit_amd import _cabi
    from gptq_gguf_toolkit_amd.ops import _DT, _ptr, _stream
    src, rows = packed_weight(ops, t, R, C, seed=2000 + t + R + C, scale=0.02, offset=OFFSET.get(t, 0),
                              gather=(R > 1 and t in (Q3, Q8)))
    packed = src.view(R, -1).cpu().numpy()
    if rows is not None:
        packed = packed[rows.cpu().numpy()]
    _, xf = activations(T, C, dt, seed=T + C)
    q = spec.quantize(xf)
    xq, xd, xbsum = on_device(*q)
    buf, y = guarded_y(T, R, dt)
    _cabi.check(_cabi.lib().gq_linear_packed_a8(t, _ptr(src), _ptr(rows), R, C, _ptr(xq), _ptr(xd), _ptr(xbsum), T, _ptr(y),
                                                _DT[dt], _stream(xq)), "gq_linear_packed_a8")
    ref, mag = spec.terms(t, packed, *q)
    err, bound = np.abs(y.double().cpu().numpy() - ref), bound2(t, ref, mag, C, dt)
    worst = float((err / bound).max())
    print(f"T={T} R={R} C={C} q_type {t} {dt}: max err / bound = {worst:.3f}")
    assert guards_intact(buf), "written outside [y, y + T * R * 2)"
    assert bool((err <= bound).all()), f"max err / bound = {worst}"
    again = ops.linear_packed_a8(t, src, xq, xd, xbsum, row_src=rows, out_dtype=dt)
    assert torch.equal(bits(again), bits(y))


# ------------------------------------------------------------------------------------------------ 3: end to end against fp64
@pytest.mark.parametrize("t", [Q4, Q6], ids=["q4k-mins", "q6k-groups-of-16"])
def test_quantize_then_gemm_against_fp64_on_the_unquantized_x(ops, t):
    """|y - x W^T| <= sum_c |w_rc| xd[t, c / 256] / 2 (a code is at most half a step from its value) + the bound of test 2."""
    T, R, C, dt = 37, 130, 768, F16
    src, _ = packed_weight(ops, t, R, C, seed=3000 + t, scale=0.02, offset=OFFSET.get(t, 0))
    packed = src.view(R, -1).cpu().numpy()
    x, xf = activations(T, C, dt, seed=5)
    y = ops.linear_packed_q8(t, src, x)
    q = spec.quantize(xf)
    W = spec.decode64(t, packed, C)
    ref2, mag = spec.terms(t, packed, *q)
    bound = np.repeat(q[1].astype(np.float64), 256, axis=1) @ np.abs(W).T / 2 + bound2(t, ref2, mag, C, dt)
    err = np.abs(y.double().cpu().numpy() - xf.astype(np.float64) @ W.T)
    worst = float((err / bound).max())
    print(f"q_type {t}: end to end max err / bound = {worst:.3f}")
    assert y.shape == (T, R) and y.dtype == dt and bool((err <= bound).all()), f"max err / bound = {worst}"


# ------------------------------------------------------------------------------------------------ 4: PackedLinear(act="q8")
def test_packed_linear_act_q8_routes_prefill_only(ops):
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    R, C = 130, 512
    src, _ = packed_weight(ops, Q4, R, C, seed=4000, scale=0.02)
    fp, q8 = PackedLinear(C, R), PackedLinear(C, R, act="q8")
    for m in (fp, q8):
        m.set_level(src, Q4)
    x20, _ = activations(20, C, F16, seed=6)
    assert torch.equal(bits(q8(x20)), bits(ops.linear_packed_q8(Q4, src, x20)))
    assert not torch.equal(bits(q8(x20)), bits(fp(x20)))
    assert torch.equal(bits(q8(x20[:1])), bits(fp(x20[:1])))  # a decode step: the GEMV on either


# ------------------------------------------------------------------------------------------------ 5: the tiny Llama .gguf
def test_ppleval_packed_act_q8(gguf_model):  # noqa: F811
    name = gguf_model["ids_pt"]
    fp, _ = run_ppleval(gguf_model, "a8_fp", "--gguf", gguf_model["gguf"], "--packed", "--packed_act", "fp")
    q8, scored = run_ppleval(gguf_model, "a8_q8", "--gguf", gguf_model["gguf"], "--packed", "--packed_act", "q8")
    a, b = fp["perplexity_results"][name], q8["perplexity_results"][name]
    print(f"perplexity --packed_act fp {a!r}, q8 {b!r}")
    assert np.isfinite(b) and b > 1 and a != b
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    assert {m.act for m in scored.modules() if isinstance(m, PackedLinear)} == {"q8"}
