"""-m gpu: the Q8_0 KV cache in a model (packed_kv_cache.py, generate --kv_cache q8_0) on the small quantized Llama of
tests/test_gpu_eval.py.  The teacher-forced 48 + 16 token run with Q8KVCache installed is held against the same run on a
fake-quant DynamicCache -- the model's ordinary attention over dequantize(quantize(K, V)) -- so that the effect of quantizing
the cache cancels and the kernels remain: the two are independently rounded 16-bit paths and differ within 2 x floor, the
fixture's dense 16-bit incremental run against the fp32 full forward."""
import io
import json
from contextlib import redirect_stdout

import pytest

from test_gpu_eval import gguf_model  # noqa: F401  (the fixture that builds the .gguf)
from test_gpu_generate import N_NEW, N_PROMPT, world  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _fake_quant_cache():
    from transformers.cache_utils import Cache, DynamicLayer
    from gptq_gguf_toolkit_amd import ops

    class FakeQ8Layer(DynamicLayer):
        """stores dequantize_blocks(quantize_q8_0(rows)); the prefill on the empty cache attends over the fresh rows"""
        def update(self, key_states, value_states, *args, **kwargs):
            empty = self.get_seq_length() == 0
            fq = [ops.dequantize_blocks(8, ops.quantize_q8_0(x.reshape(-1, x.shape[-1])), x.dtype).view(x.shape)
                  for x in (key_states, value_states)]
            stored = super().update(*fq, *args, **kwargs)
            return (key_states, value_states) if empty else stored

    return Cache(layer_class_to_replicate=FakeQ8Layer)


@torch.no_grad()
def _teacher_forced(model, ids, past):
    out = model(input_ids=ids[:, :N_PROMPT], past_key_values=past, use_cache=True)
    rows = []
    for i in range(N_PROMPT, ids.shape[1]):
        out = model(input_ids=ids[:, i:i + 1], past_key_values=past, use_cache=True)
        rows.append(out.logits[:, -1])
    return torch.stack(rows, 1).float()


@pytest.mark.parametrize("which", ["dense", "packed"])
def test_q8_cache_equals_the_fake_quant_cache_within_16_bit_noise(world, monkeypatch, which):  # noqa: F811
    from gptq_gguf_toolkit_amd import ops, packed_kv_cache as pk
    model, ids = world[which], world["ids0"]
    want = _teacher_forced(model, ids, _fake_quant_cache())
    calls, real, real_sdpa = [], ops.attn_decode_q8_0, torch.nn.functional.scaled_dot_product_attention
    monkeypatch.setattr(ops, "attn_decode_q8_0", lambda q, *a, **k: (calls.append(("kernel", q.shape[2])), real(q, *a, **k))[1])
    monkeypatch.setattr(pk.torch.nn.functional, "scaled_dot_product_attention",
                        lambda q, *a, **k: (calls.append(("fallback", q.shape[2])), real_sdpa(q, *a, **k))[1])
    before = model.config._attn_implementation
    cache = pk.install(model, pk.Q8KVCache(model.config, 1, N_PROMPT, device=ids.device))  # (grows once, at token 49)
    try:
        assert model.config._attn_implementation == pk.ATTN_NAME
        got = _teacher_forced(model, ids, cache)
    finally:
        pk.restore(model)
    monkeypatch.undo()
    assert model.config._attn_implementation == before and not hasattr(model, "_gq_q8_prev_attn")
    layers = model.config.num_hidden_layers
    assert calls == [("fallback", N_PROMPT)] * layers + [("kernel", 1)] * (layers * N_NEW)
    assert cache.get_seq_length() == N_PROMPT + N_NEW and cache.layers[0].capacity == 2 * N_PROMPT
    err = float((got - want).abs().max())
    print(f"{which}: Q8KVCache against the fake-quant DynamicCache, 16 x 512 logits: {err!r}; floor {world['floor']!r}; the "
          f"fake-quant run against the fp32 reference {float((want - world['ref']).abs().max())!r}")
    assert bool(torch.isfinite(got).all()) and err <= 2 * world["floor"]


def test_generate_command_line_with_the_q8_cache(world):  # noqa: F811
    from gptq_gguf_toolkit_amd import generate
    out = world["tmp"] / "gen_q8kv.json"
    argv = ["--model_name_or_path", world["hf"], "--gguf", world["gguf"], "--packed", "--prompt_ids", world["ids_pt"],
            "--max_new_tokens", "8", "--dtype", "float16", "--kv_cache", "q8_0", "--output_file", str(out)]
    with redirect_stdout(io.StringIO()):
        generate.main(argv)
    res = json.loads(out.read_text())
    assert len(res["prompts"]) == 3
    for rec in res["prompts"]:
        assert len(rec["new_ids"]) == 8 and all(0 <= i < 512 for i in rec["new_ids"])
