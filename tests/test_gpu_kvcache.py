"""-m gpu: the Q8_0 KV cache kernels (include/gptq_gguf_kvcache.h).  The append must be the Q8_0 encoder byte for
byte and touch nothing else; the split-KV decode attention is held against an fp64 attention over the decoded cache, with
torch's own 16-bit SDPA (math backend) on the same decoded cache as the floor: two independently rounded 16-bit paths may
differ by 2x (the margin of tests/test_gpu_generate.py); and the same call twice gives the same bits."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"


def _cache(B, Hkv, S_cap, D, fill=0xA5):
    return torch.full((B, Hkv, S_cap, D // 32 * 34), fill, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("T,pos0", [(1, 0), (1, 3), (5, 0), (5, 3)])
def test_append_is_the_encoder_and_touches_nothing_else(D, dtype, T, pos0):
    from gptq_gguf_toolkit_amd import ops
    B, Hkv, S_cap = 2, 3, 12
    g = torch.Generator(device=DEV).manual_seed(D + T + pos0)
    k, v = (torch.randn(B, T, Hkv, D, generator=g, device=DEV).mul(s).to(dtype).transpose(1, 2) for s in (1.0, 3.0))  # the layer's view
    assert not k.is_contiguous() or T == 1
    kc, vc = _cache(B, Hkv, S_cap, D), _cache(B, Hkv, S_cap, D)
    ops.kv_append_q8_0(kc, vc, k, v, pos0)
    for c, x in ((kc, k), (vc, v)):
        want = _cache(B, Hkv, S_cap, D)
        want[:, :, pos0:pos0 + T] = ops.quantize_q8_0(x.reshape(-1, D)).view(B, Hkv, T, -1)
        assert torch.equal(c, want)


def _case(D, G, T, B, S, dtype, outlier=False, Hkv=1, seed=0):
    """a filled cache of S positions, the query of its last T, kv_start = [0, 5] (capped at pos0)"""
    from gptq_gguf_toolkit_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed + 1000 * S + D + G)
    pos0, S_cap = S - T, (S + 3) // 4 * 4
    k, v = (torch.randn(B, Hkv, S, D, generator=g, device=DEV).to(dtype) for _ in range(2))
    q = torch.randn(B, T, Hkv * G, D, generator=g, device=DEV).to(dtype).transpose(1, 2)
    if outlier:  # one score of about +30 far from the first chunk: the running max moves late, across chunks
        p = S - S // 3
        k[:, :, p] = (q[:, ::G, -1].float() * (30.0 * D ** 0.5 / q[:, ::G, -1].float().pow(2).sum(-1, keepdim=True))).to(dtype)
    kc, vc = torch.empty(B, Hkv, S_cap, D // 32 * 34, dtype=torch.uint8, device=DEV), None
    vc = torch.empty_like(kc)
    kc.view(torch.int16).fill_(0x7e00), vc.view(torch.int16).fill_(0x7e00)  # rows past S decode to NaN: they must not count
    ops.kv_append_q8_0(kc, vc, k, v, 0)
    start = torch.tensor([0, 5][:B], dtype=torch.int32, device=DEV).clamp(max=pos0)
    return q, kc, vc, pos0, start


def _reference(q, kc, vc, pos0, start, scale, dtype):
    """(fp64 attention, 16-bit math SDPA) over the cache decoded by dequantize_blocks, same mask"""
    from gptq_gguf_toolkit_amd import ops
    B, Hq, T, D = q.shape
    Hkv, S = kc.shape[1], pos0 + T
    kd, vd = (ops.dequantize_blocks(8, c[:, :, :S].reshape(-1, c.shape[3]), dtype).view(B, Hkv, S, D).repeat_interleave(Hq // Hkv, 1)
              for c in (kc, vc))
    pos = torch.arange(S, device=DEV)
    mask = (pos[None, None, :] <= (pos0 + torch.arange(T, device=DEV))[None, :, None]) & (pos[None, None, :] >= start[:, None, None])
    mask = mask[:, None]  # [B, 1, T, S]
    s = (q.double() @ kd.double().transpose(-1, -2)) * scale
    ref = torch.softmax(s.masked_fill(~mask, float("-inf")), -1) @ vd.double()
    with torch.nn.attention.sdpa_kernel(torch.nn.attention.SDPBackend.MATH):
        low = torch.nn.functional.scaled_dot_product_attention(q, kd, vd, attn_mask=mask, scale=scale)
    return ref.transpose(1, 2), low.transpose(1, 2)


def _plan_lengths():
    """from the plan's constants: one chunk -+ 1, three chunks, the length of a second turn of a wave's loop"""
    from gptq_gguf_toolkit_amd import ops
    p = ops.attn_decode_plan(1, 2, 1, 1)
    three = 2 * p["min_chunk"] + 1
    assert ops.attn_decode_plan(three, 2, 1, 1)["splits"] >= 3 and ops.attn_decode_plan(p["min_chunk"], 2, 1, 1)["splits"] == 1
    return p["min_chunk"], three, p["turn"] + 1


# D, G, T, S, dtype, outlier -- S by name for the lengths taken from the plan
CASES = [(64, 1, 1, 1, "f16", False), (128, 4, 1, 31, "bf16", False), (128, 4, 1, 32, "f16", False), (64, 8, 1, 33, "bf16", False),
         (64, 4, 3, 33, "f16", False), (128, 8, 3, 40, "bf16", False), (128, 8, 3, "three", "f16", False),
         (128, 4, 1, "chunk-1", "bf16", False), (64, 1, 3, "chunk", "f16", False), (128, 1, 1, "chunk+1", "bf16", False),
         (64, 8, 1, "three", "bf16", True), (128, 4, 3, "turn", "f16", False), (64, 4, 1, "turn", "bf16", False)]


@pytest.mark.parametrize("D,G,T,S,dt,outlier", CASES)
def test_attention_against_fp64_within_twice_the_16_bit_floor(D, G, T, S, dt, outlier):
    from gptq_gguf_toolkit_amd import ops
    chunk, three, turn = _plan_lengths()
    S = {"three": three, "chunk-1": chunk - 1, "chunk": chunk, "chunk+1": chunk + 1, "turn": turn}.get(S, S)
    dtype = torch.float16 if dt == "f16" else torch.bfloat16
    B, scale = 2, D ** -0.5
    q, kc, vc, pos0, start = _case(D, G, T, B, S, dtype, outlier)
    ref, low = _reference(q, kc, vc, pos0, start, scale, dtype)
    out = torch.full((B, T, G, D), float("nan"), dtype=dtype, device=DEV)
    ops.attn_decode_q8_0(q, kc, vc, pos0, scale, start, out=out)
    assert not torch.isnan(out).any()  # every element is written, and no row past S was counted
    floor, err = float((low.double() - ref).abs().max()), float((out.double() - ref).abs().max())
    ratio = err / floor if floor > 0 else float("inf") * err if err else 0.0  # (S = 1: the output is V's row, both errors are 0)
    print(f"attn_decode_q8_0 D={D} G={G} T={T} S={S} {dt} outlier={outlier}: floor {floor:.3e} kernel {err:.3e} ratio {ratio:.2f}")
    assert err <= 2 * floor
    again = ops.attn_decode_q8_0(q, kc, vc, pos0, scale, start)
    assert torch.equal(again.view(torch.int16), out.view(torch.int16))  # deterministic: the same bits
    if not start.any():
        return
    free = ops.attn_decode_q8_0(q, kc, vc, pos0, scale, None)  # kv_start NULL is kv_start 0: row 0 of the batch has none
    assert torch.equal(free[0].view(torch.int16), out[0].view(torch.int16))
