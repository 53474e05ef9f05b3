"""-m gpu: the chunked prefill on the packed KV cache in a model (Q8KVCache(prefill="q8_0"), generate --kv_prefill q8_0
--prefill_chunk N) on the small quantized Llama of tests/test_gpu_generate.py.  The prompt goes in two pieces, the second of
more columns than the decode kernel takes, then the teacher-forced decode steps; the same run on the fake-quant DynamicCache of
tests/test_gpu_kvcache_model.py is the comparison, within 2 x floor as there."""
import io
import json
from contextlib import redirect_stdout

import pytest

from test_gpu_eval import gguf_model  # noqa: F401  (the fixture that builds the .gguf)
from test_gpu_generate import N_NEW, N_PROMPT, world  # noqa: F401
from test_gpu_kvcache_model import _fake_quant_cache

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
FIRST = 12  # tokens of the first piece; the second has N_PROMPT - FIRST = 36 > 64 / G = 32


@torch.no_grad()
def _two_pieces_then_decode(model, ids, past):
    for piece in (ids[:, :FIRST], ids[:, FIRST:N_PROMPT]):
        model(input_ids=piece, past_key_values=past, use_cache=True)
    rows = [model(input_ids=ids[:, i:i + 1], past_key_values=past, use_cache=True).logits[:, -1] for i in range(N_PROMPT, ids.shape[1])]
    return torch.stack(rows, 1).float()


@pytest.mark.parametrize("which", ["dense", "packed"])
def test_chunked_prefill_on_the_packed_cache_equals_the_fake_quant_cache(world, monkeypatch, which):  # noqa: F811
    from gptq_gguf_toolkit_amd import ops, packed_kv_cache as pk
    model, ids = world[which], world["ids0"]
    cfg = model.config
    assert cfg.num_attention_heads // cfg.num_key_value_heads * (N_PROMPT - FIRST) > ops.ATTN_DECODE_MAX_COLS
    want = _two_pieces_then_decode(model, ids, _fake_quant_cache())
    calls, real, real_sdpa = [], ops.attn_prefill_q8_0, torch.nn.functional.scaled_dot_product_attention
    monkeypatch.setattr(ops, "attn_prefill_q8_0", lambda q, *a, **k: (calls.append(("prefill", q.shape[2])), real(q, *a, **k))[1])
    monkeypatch.setattr(pk.torch.nn.functional, "scaled_dot_product_attention",
                        lambda q, *a, **k: (calls.append(("sdpa", q.shape[2])), real_sdpa(q, *a, **k))[1])
    got = {}
    for prefill in ("q8_0", "sdpa"):
        calls.clear()
        cache = pk.install(model, pk.Q8KVCache(cfg, 1, ids.shape[1], device=ids.device, prefill=prefill))
        try:
            got[prefill] = _two_pieces_then_decode(model, ids, cache)
        finally:
            pk.restore(model)
        second = "prefill" if prefill == "q8_0" else "sdpa"  # the first piece attends over its fresh rows either way
        assert calls == [("sdpa", FIRST)] * cfg.num_hidden_layers + [(second, N_PROMPT - FIRST)] * cfg.num_hidden_layers
    err = float((got["q8_0"] - want).abs().max())
    print(f"{which}: two-piece prefill on Q8KVCache(prefill='q8_0') against the fake-quant DynamicCache, 16 x 512 logits: {err!r}; "
          f"floor {world['floor']!r}; prefill='sdpa' {float((got['sdpa'] - want).abs().max())!r}")
    assert bool(torch.isfinite(got["q8_0"]).all()) and err <= 2 * world["floor"]


def test_generate_command_line_with_the_chunked_q8_prefill(world):  # noqa: F811
    from gptq_gguf_toolkit_amd import generate
    out = world["tmp"] / "gen_q8prefill.json"
    argv = ["--model_name_or_path", world["hf"], "--gguf", world["gguf"], "--packed", "--prompt_ids", world["ids_pt"],
            "--max_new_tokens", "8", "--dtype", "float16", "--kv_cache", "q8_0", "--kv_prefill", "q8_0", "--prefill_chunk", "24",
            "--output_file", str(out)]
    with redirect_stdout(io.StringIO()):
        generate.main(argv)
    res = json.loads(out.read_text())
    assert len(res["prompts"]) == 3
    for rec in res["prompts"]:
        assert len(rec["new_ids"]) == 8 and all(0 <= i < 512 for i in rec["new_ids"])
