"""The grouped dense decode launch on int8 activations (K39): gq_gemv_packed_group_a8 against fp64 under K37's derived bound
(tests/test_gpu_qgemv_a8.py: the per-row arithmetic is the same) and bit for bit against gq_gemv_packed_a8 per member, the
second turn of a member's share of the grid, the SwiGLU form against ops.fwd_silu_mul of the two single launches, and
generate --decode_group on against off on the tiny Llama."""
import numpy as np
import pytest

import act_q8_spec as spec
from test_gpu_eval import gguf_model  # noqa: F401  (the fixture that builds the small .gguf)
from test_gpu_generate import N_PROMPT, world  # noqa: F401  (world: that file and its evaluation ids)
from test_gpu_qgemm import BF16, F16, FILL, Q2, Q3, Q4, Q5, Q6, Q8, bits, guarded_y, guards_intact, ops, packed_weight  # noqa: F401
from test_gpu_qgemm_a8 import OFFSET, activations, bound2

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SPLIT, SWIGLU = 0, 1
# row counts that are no multiples of 16: a member's last row group is partial, and one workgroup per member is the least
SETS = {"q4q6q8": ((Q4, 40), (Q6, 17), (Q8, 5)), "q2q3q5": ((Q2, 1), (Q3, 130), (Q5, 16)), "alone": ((Q6, 19),)}
CASES = [(T, C, s, (F16, BF16)[i % 2]) for i, (T, C, s) in enumerate((T, C, s) for T in (1, 3, 4) for C in (256, 2816) for s in SETS)]
CASES += [(2, 4352, "q4q6q8", BF16)]  # 17 superblocks: a wave's second step over the row, partial


def weights(ops, members, C, seed):
    """[(q_type, blocks, row_src, R)]; Q3_K and Q8_0 carry a row gather, the 2-byte aligned types lie at byte +2."""
    return [(t, *packed_weight(ops, t, R, C, seed=seed + 7 * i + t, scale=0.02, offset=OFFSET.get(t, 0), gather=(R > 1 and t in (Q3, Q8))), R)
            for i, (t, R) in enumerate(members)]


def raw_group(ms, x, ys, mode=SPLIT):
    from gptq_gguf_toolkit_amd import _cabi
    from gptq_gguf_toolkit_amd.ops import _DT, _ptr, _stream
    tab = (_cabi.GemvMember * len(ms))(*[_cabi.GemvMember(t, _ptr(src), _ptr(rows), R, _ptr(y)) for (t, src, rows, R), y in zip(ms, ys)])
    _cabi.check(_cabi.lib().gq_gemv_packed_group_a8(tab, len(ms), x.shape[-1], _ptr(x), x.shape[0], _DT[x.dtype], mode, _stream(x)),
                "gq_gemv_packed_group_a8")


# ------------------------------------------------------------------------------------------------ 1: SPLIT against fp64
@pytest.mark.parametrize("T,C,name,dt", CASES, ids=[f"T{c[0]}-C{c[1]}-{c[2]}-{str(c[3])[6:]}" for c in CASES])
def test_split_against_fp64_and_bit_for_bit_against_the_single_launch(ops, T, C, name, dt):
    ms = weights(ops, SETS[name], C, seed=6000 + C)
    x, xf = activations(T, C, dt, seed=T + C)
    act = spec.quantize(xf)
    bufs = [guarded_y(T, R, dt) for *_, R in ms]
    raw_group(ms, x, [y for _, y in bufs])
    outs = ops.gemv_packed_group_q8([m[:3] for m in ms], x)
    for (t, src, rows, R), (buf, y), out in zip(ms, bufs, outs):
        packed = src.view(R, -1).cpu().numpy()
        ref, mag = spec.terms(t, packed if rows is None else packed[rows.cpu().numpy()], *act)
        err, bound = np.abs(y.double().cpu().numpy() - ref), bound2(t, ref, mag, C, dt)
        print(f"T={T} C={C} q_type {t} R={R} {dt}: max err / bound = {float((err / bound).max()):.3f}")
        assert guards_intact(buf), "written outside [y, y + T * R * 2)"
        assert bool((err <= bound).all())
        assert torch.equal(bits(y), bits(ops.gemv_packed_q8(t, src, x, rows))) and torch.equal(bits(out), bits(y))


# ------------------------------------------------------------------------------------------------ 2: the second turn
def test_a_member_whose_share_of_the_grid_takes_a_second_and_a_third_turn(ops):
    T, C, dt, small = 2, 256, BF16, ((Q6, 24), (Q4, 40))
    types, tail = [Q4, Q6, Q4], [24, 40]
    share = ops.gemv_group_a8_plan(types, [3 * 256 * 16] + tail, C, T)["first_wg"][1]  # the big member's workgroups on a capped grid
    R_big = 2 * share * 16 + 16 + 5  # two whole turns; in the third, workgroup 0 a whole row group and workgroup 1 five rows
    plan = ops.gemv_group_a8_plan(types, [R_big] + tail, C, T)
    assert plan["grid"] == 256 and plan["first_wg"] == [0, share, 255, 256] and plan["fits"]
    ms = weights(ops, ((Q4, R_big),) + small, C, seed=7000)
    x, _ = activations(T, C, dt, seed=11)
    for (t, src, rows, R), y in zip(ms, ops.gemv_packed_group_q8([m[:3] for m in ms], x)):
        assert torch.equal(bits(y), bits(ops.gemv_packed_q8(t, src, x, rows))), (t, R)


# ------------------------------------------------------------------------------------------------ 3: SWIGLU
SW = [(t, R, T, C, (F16, BF16)[i % 2]) for i, (t, R, T, C) in enumerate((t, R, T, C) for t in (Q4, Q6) for R in (1, 19, 130) for T in (1, 4) for C in (256, 2816))]


@pytest.mark.parametrize("t,R,T,C,dt", SW, ids=[f"q{c[0]}-R{c[1]}-T{c[2]}-C{c[3]}-{str(c[4])[6:]}" for c in SW])
def test_swiglu_equals_silu_mul_of_the_two_single_launches(ops, t, R, T, C, dt):
    """ops.fwd_silu_mul is elementwise and takes a multiple of 8 elements; T * R here is none, so G and U are padded with
    zeros for that call and the padding is cut off again."""
    (_, g, _, _), (_, u, _, _) = ms = [(t, *packed_weight(ops, t, R, C, seed=8000 + s + R + C, scale=0.02, offset=OFFSET.get(t, 0)), R) for s in (0, 1)]
    x, _ = activations(T, C, dt, seed=T + C + 1)
    pad = [0, -(T * R) % 8]
    G, U = (torch.nn.functional.pad(ops.gemv_packed_q8(t, w, x).reshape(-1), pad) for w in (g, u))
    want = ops.fwd_silu_mul(G, U)[:T * R].view(T, R)
    buf, both = guarded_y(2 * T, R, dt)  # act, and behind it the [T, R] a second output would take
    raw_group(ms, x, [both[:T], None], SWIGLU)
    assert torch.equal(bits(both[:T]), bits(want)) and guards_intact(buf)
    assert bool((bits(both[T:]) == FILL).all()), "written where U would have been"
    assert torch.equal(bits(ops.gemv_swiglu_packed_q8(t, g, u, x)), bits(want))


# ------------------------------------------------------------------------------------------------ 4: the tiny Llama .gguf
@torch.no_grad()
def steps(model, ids, sizes):
    """Teacher-forced: prefill ids[:, :48], then one forward per piece of `sizes` tokens -> the logits of every piece, stacked."""
    out, at, rows = model(input_ids=ids[:, :N_PROMPT], use_cache=True), N_PROMPT, []
    for n in sizes:
        out = model(input_ids=ids[:, at:at + n], past_key_values=out.past_key_values, use_cache=True)
        rows.append(out.logits[0])
        at += n
    return torch.cat(rows).float()


def test_generate_decode_group_on_equals_off(world, monkeypatch):  # noqa: F811
    """The file's gate (Q6_K) and up (Q4_K) differ in type, so as loaded its MLPs take the SPLIT launch and fwd_silu_mul: two
    group calls per layer and step.  With up switched to gate's level in both models the pair is of one type: one group call
    (q / k / v) and one SwiGLU call per layer and step.  Levels are read at call time: no reinstall."""
    from gptq_gguf_toolkit_amd import generate, ops, ppleval
    base = ["--model_name_or_path", world["hf"], "--gguf", world["gguf"], "--packed", "--decode_act", "q8", "--prompt_ids",
            world["ids_pt"], "--max_new_tokens", "8", "--dtype", "float16", "--attn_implementation", "eager", "--output_file", "-"]
    off, on = (ppleval.apply_weights(ppleval.load_hf_model(a, torch.device("cuda")), a)
               for a in (generate.parse_args(base + extra) for extra in ([], ["--decode_group", "on"])))
    calls = {"gemv_packed_group_q8": 0, "gemv_swiglu_packed_q8": 0}
    for name in calls:
        def counted(*a, _real=getattr(ops, name), _name=name):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(ops, name, counted)
    layers, ids = on.config.num_hidden_layers, world["ids0"]
    for same_type in (False, True):
        if same_type:
            for model in (off, on):
                for layer in model.model.layers:
                    layer.mlp.up_proj.set_level(layer.mlp.gate_proj.blocks, layer.mlp.gate_proj.q_type)
        for sizes, grouped in (([1] * 8 + [3], 9), ([5], 0)):  # 5 tokens are beyond GEMV_A8_MAX_T: no group call
            calls.update(dict.fromkeys(calls, 0))
            want = steps(off, ids, sizes)
            assert sum(calls.values()) == 0
            assert torch.equal(steps(on, ids, sizes), want) and bool(torch.isfinite(want).all())
            assert calls == {"gemv_packed_group_q8": layers * grouped * (1 if same_type else 2),
                             "gemv_swiglu_packed_q8": layers * grouped * (1 if same_type else 0)}, (same_type, sizes, calls)
