"""The packed decode step on int8 activations (K37): gq_gemv_packed_a8 against fp64 on tests/act_q8_spec.py's quantized
activations, the second turn of its grid-stride loop, its refusals, PackedLinear(decode_act="q8") and generate --decode_act q8
on the tiny Llama.  The bound is tests/test_gpu_qgemm_a8.py's, derived from the roundings include/gptq_gguf_qgemm_a8.h lists:
include/gptq_gguf_qgemv_a8.h has the same operations per term and another order of the same C / 256 additions (Q8_0: of the
same eight per superblock), and the bound holds for any order."""
import numpy as np
import pytest

import act_q8_spec as spec
from test_gpu_eval import gguf_model  # noqa: F401  (the fixture that builds the small .gguf)
from test_gpu_generate import incremental, world  # noqa: F401  (world: that file loaded dense and packed, K22's fp16 floor)
from test_gpu_qgemm import BF16, F16, Q3, Q4, Q6, Q8, TYPES, bits, guarded_y, guards_intact, ops, packed_weight  # noqa: F401
from test_gpu_qgemm_a8 import OFFSET, activations, bound2

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

IQ4_NL = 20
GRID = [(T, R, C) for T in (1, 3, 4) for R in (1, 130) for C in (256, 2816)]
CASES = [(T, R, C, TYPES[i % 6], (F16, BF16)[(i + i // 6) % 2]) for i, (T, R, C) in enumerate(GRID)]  # every type in both dtypes
CASES += [(2, 19, 4352, TYPES[0], BF16), (2, 19, 4352, Q6, F16)]  # 17 superblocks: a wave's second step over the row, partial


def check_against_fp64(ops, t, src, rows, R, C, x, xf, dt):
    """One raw call into a guarded y -> y; asserts the bound, the guards and that ops.gemv_packed_q8 repeats the bits."""
    from gptq_gguf_toolkit_amd import _cabi
    from gptq_gguf_toolkit_amd.ops import _DT, _ptr, _stream
    T = x.shape[0]
    packed = src.view(R, -1).cpu().numpy()
    if rows is not None:
        packed = packed[rows.cpu().numpy()]
    buf, y = guarded_y(T, R, dt)
    _cabi.check(_cabi.lib().gq_gemv_packed_a8(t, _ptr(src), _ptr(rows), R, C, _ptr(x), T, _DT[dt], _ptr(y), _stream(x)),
                "gq_gemv_packed_a8")
    ref, mag = spec.terms(t, packed, *spec.quantize(xf))
    err, bound = np.abs(y.double().cpu().numpy() - ref), bound2(t, ref, mag, C, dt)
    worst, at = float((err / bound).max()), int((err / bound).argmax())
    print(f"T={T} R={R} C={C} q_type {t} {dt}: max err / bound = {worst:.3f} (where ref = {ref.flat[at]!r})")
    assert guards_intact(buf), "written outside [y, y + T * R * 2)"
    assert bool((err <= bound).all()), f"max err / bound = {worst}"
    assert torch.equal(bits(ops.gemv_packed_q8(t, src, x, rows)), bits(y))
    return y


# ------------------------------------------------------------------------------------------------ 1: against fp64
@pytest.mark.parametrize("T,R,C,t,dt", CASES, ids=[f"T{c[0]}-R{c[1]}-C{c[2]}-q{c[3]}-{str(c[4])[6:]}" for c in CASES])
def test_gemv_against_fp64_on_the_spec_quantized_activations(ops, T, R, C, t, dt):
    """|y - ref| <= u_out |ref| + (C/256 + 4, Q8_0: 12) 2^-24 mag + 2^-149 with ref = spec.terms(spec.quantize(x)): the kernel's
    own quantizer must give the spec's codes -- one wrong code fails the bound."""
    src, rows = packed_weight(ops, t, R, C, seed=2000 + t + R + C, scale=0.02, offset=OFFSET.get(t, 0),
                              gather=(R > 1 and t in (Q3, Q8)))
    x, xf = activations(T, C, dt, seed=T + C)
    if C > 256:
        x[T - 1, 512:768] = 0                       # an all-zero superblock: d = 0, codes 0
        x[0, 300] = -x[0, 256:512].abs().max() * 2  # a superblock whose maximum is negative
        xf = x.float().cpu().numpy()
    check_against_fp64(ops, t, src, rows, R, C, x, xf, dt)


# ------------------------------------------------------------------------------------------------ 2: the second turn
@pytest.mark.parametrize("t", [Q4, Q6], ids=["q4k-16-byte", "q6k-2-byte"])
def test_rows_of_a_second_turn_equal_the_same_rows_called_alone(ops, t):
    # bf16: the bound's u_out |ref| is a relative rounding, which an fp16 SUBNORMAL output (|y| < 2^-14, spacing 2^-24) does
    # not have; with one term per output, 8234 outputs of standard deviation 0.3 hold one or two of them.
    T, C, dt = 2, 256, BF16
    plan = ops.gemv_a8_plan(T, 1, C)
    first = plan["grid_cap"] * plan["rows_per_turn"]  # rows of the first turn of a full grid
    R = first + plan["rows_per_turn"] + 5             # workgroup 0 takes a whole second turn, workgroup 1 five rows of one
    assert ops.gemv_a8_plan(T, R, C)["grid"] == plan["grid_cap"] and plan["fits"]
    src, _ = packed_weight(ops, t, R, C, seed=5000 + t, scale=0.02, offset=OFFSET.get(t, 0))
    x, xf = activations(T, C, dt, seed=9)
    y = check_against_fp64(ops, t, src, None, R, C, x, xf, dt)
    lo = first - 3
    alone = ops.gemv_packed_q8(t, src.view(R, -1)[lo:], x)  # the same rows as turn 0 of another grid
    assert torch.equal(bits(alone), bits(y[:, lo:]))


# ------------------------------------------------------------------------------------------------ 3: refusals and routing
def test_refusals_and_packed_linear_routes(ops):
    from gptq_gguf_toolkit_amd._cabi import GQError
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    R, C = 130, 512
    src, _ = packed_weight(ops, Q4, R, C, seed=4000, scale=0.02)
    x5, _ = activations(5, C, F16, seed=6)
    with pytest.raises(GQError, match="T=5"):
        ops.gemv_packed_q8(Q4, src, x5)
    nl = torch.zeros(R * (C // 32) * 18, dtype=torch.uint8, device="cuda")  # IQ4_NL blocks with d = 0
    with pytest.raises(GQError, match="q_type 20"):
        ops.gemv_packed_q8(IQ4_NL, nl, x5[:1])
    big = 32768
    assert not ops.gemv_a8_plan(4, 1, big)["fits"] and ops.gemv_a8_plan(4, 1, 14336)["fits"] and ops.gemv_a8_plan(1, 1, 28672)["fits"]
    with pytest.raises(GQError, match=f"T=4 C={big}"):
        ops.gemv_packed_q8(Q4, torch.zeros(big // 256 * 144, dtype=torch.uint8, device="cuda"), torch.zeros(4, big, dtype=F16, device="cuda"))

    fp, q8, both = PackedLinear(C, R), PackedLinear(C, R, decode_act="q8"), PackedLinear(C, R, act="q8", decode_act="q8")
    for m in (fp, q8, both):
        m.set_level(src, Q4)
    assert "decode_act=q8" in repr(q8) and "decode_act=fp" in repr(fp)
    for T in (1, 4):
        assert torch.equal(bits(q8(x5[:T])), bits(ops.gemv_packed_q8(Q4, src, x5[:T])))
        assert not torch.equal(bits(q8(x5[:T])), bits(fp(x5[:T])))
        assert torch.equal(bits(both(x5[:T])), bits(q8(x5[:T])))
    assert torch.equal(bits(q8(x5)), bits(ops.gemv_packed(Q4, src, x5)))        # T = 5: the 16-bit GEMV
    assert torch.equal(bits(fp(x5[:1])), bits(ops.gemv_packed(Q4, src, x5[:1])))  # the default
    q8.set_level(nl, IQ4_NL)
    assert torch.equal(bits(q8(x5[:1])), bits(ops.gemv_packed(IQ4_NL, nl, x5[:1])))
    W = torch.randn(R, C, generator=torch.Generator().manual_seed(1)).half().cuda()
    q8.set_level(W, None)
    assert torch.equal(q8(x5[:1]), torch.nn.functional.linear(x5[:1], W))


# ------------------------------------------------------------------------------------------------ 4: the tiny Llama .gguf
def test_generate_decode_act_q8(world):  # noqa: F811
    """Teacher-forced one-token steps of the model that generate --packed --decode_act q8 builds.  max |q8 - fp| is printed
    beside K22's fp16 floor and recorded in DESIGN K37; it is not asserted (int8 activations are other numerics)."""
    from gptq_gguf_toolkit_amd import generate, ppleval
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    argv = ["--model_name_or_path", world["hf"], "--gguf", world["gguf"], "--packed", "--decode_act", "q8", "--prompt_ids",
            world["ids_pt"], "--max_new_tokens", "8", "--dtype", "float16", "--attn_implementation", "eager", "--output_file", "-"]
    args = generate.parse_args(argv)
    model = ppleval.apply_weights(ppleval.load_hf_model(args, torch.device("cuda")), args)
    mods = [m for m in model.modules() if isinstance(m, PackedLinear)]
    assert mods and {m.decode_act for m in mods} == {"q8"} and {m.act for m in mods} == {"fp"}
    q8, fp = incremental(model, world["ids0"]), incremental(world["packed"], world["ids0"])
    print(f"teacher-forced decode, 16 x 512 logits: max |q8 - fp| {float((q8 - fp).abs().max())!r}, q8 against fp32 "
          f"{float((q8 - world['ref']).abs().max())!r}, K22's fp16 floor {world['floor']!r}")
    assert bool(torch.isfinite(q8).all()) and not torch.equal(q8, fp)
    assert generate.greedy(model, world["ids0"][:, :48], 4).shape == (1, 52)
