"""-m gpu: the prefill attention on the Q8_0 KV cache (include/gptq_gguf_kvprefill.h) against the fp64 attention
over the decoded cache, with torch's 16-bit math SDPA on the same decoded cache as the floor (the rule and the helpers of
tests/test_gpu_kvcache.py): err <= 2 floor, every element written, the same bits twice.  The lengths come from the plan."""
import pytest

from test_gpu_kvcache import DEV, _case, _reference

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# D, G, T, pos0 (in turns U and positions), dtype, outlier, kv_start of row 1 (None: _case's) -- T "C+1": block columns + 1
CASES = [(64, 1, "C+1", (0, 0), "f16", False, None),     # a second block of one column
         (128, 8, 9, (0, 0), "bf16", False, None),       # 72 columns: the case the decode call refuses
         (128, 4, 17, (1, -1), "f16", False, None),      # the diagonal crosses a turn boundary inside the chunk
         (64, 4, 20, (3, 5), "bf16", False, None),       # three full turns before the diagonal; S_cap > S
         (128, 4, 20, (3, 5), "f16", True, None),        # ... with a score of about +30 two thirds in
         (64, 2, 40, (2, 0), "bf16", False, (1, 5)),     # kv_start = [0, U + 5]: a whole turn skipped for row 1 only
         (128, 2, 40, (0, 0), "f16", False, (0, 3))]     # kv_start = [0, 3] at pos0 = 0: three padding tokens in row 1


@pytest.mark.parametrize("D,G,T,at,dt,outlier,pad", CASES)
def test_prefill_attention_against_fp64_within_twice_the_16_bit_floor(D, G, T, at, dt, outlier, pad):
    from gptq_gguf_toolkit_amd import ops
    plan = ops.attn_prefill_plan(1, 1)
    C, U = plan["block_cols"], plan["turn"]
    T = C + 1 if T == "C+1" else T
    pos0 = at[0] * U + at[1]
    dtype = torch.float16 if dt == "f16" else torch.bfloat16
    B, Hkv, scale = 2, D // 64, D ** -0.5  # (two KV heads at D = 128)
    q, kc, vc, pos0, start = _case(D, G, T, B, pos0 + T, dtype, outlier, Hkv=Hkv)
    if pad is not None:
        start = torch.tensor([0, pad[0] * U + pad[1]], dtype=torch.int32, device=DEV)
    assert G * T > ops.ATTN_DECODE_MAX_COLS and ops.attn_prefill_plan(T, G)["blocks"] == -(-G * T // C) >= 2
    ref, low = _reference(q, kc, vc, pos0, start, scale, dtype)
    out = torch.full((B, T, Hkv * G, D), float("nan"), dtype=dtype, device=DEV)
    ops.attn_prefill_q8_0(q, kc, vc, pos0, scale, start, out=out)
    assert not torch.isnan(out).any()  # every element is written, and no row past S was counted
    seen = (pos0 + torch.arange(T, device=DEV))[None] >= start[:, None]  # [B, T]: the token's own position is visible
    assert bool((out[~seen] == 0).all()) and int((~seen).sum()) == (3 if pad == (0, 3) else 0)  # padding tokens: exact zeros
    floor, err = float((low.double() - ref)[seen].abs().max()), float((out.double() - ref)[seen].abs().max())
    print(f"attn_prefill_q8_0 D={D} G={G} T={T} pos0={pos0} {dt} outlier={outlier} start={start.tolist()}: floor {floor:.3e} "
          f"kernel {err:.3e} ratio {err / floor:.2f}")
    assert err <= 2 * floor
    again = ops.attn_prefill_q8_0(q, kc, vc, pos0, scale, start)
    assert torch.equal(again.view(torch.int16), out.view(torch.int16))  # deterministic: the same bits
