"""Decoding with a packed model on the GPU: a `.gguf` loaded packed, run token by token on the HF KV cache -- every Linear of
a one-token step goes through gq_gemv_packed -- against the same file loaded dense and an fp32 copy of it; generate.greedy and
the command line.  The model is the small quantized Llama of tests/test_gpu_eval.py (loaded from its saved directory, as
that fixture explains)."""
import copy
import io
import json
import os
import sys
from contextlib import redirect_stdout

import pytest

from conftest import ROOT
from test_gpu_eval import gguf_model, load_hf  # noqa: F401  (gguf_model: the fixture that builds the .gguf)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

N_PROMPT, N_NEW, N_LINEARS = 48, 16, 14


@pytest.fixture()
def gemv_calls(monkeypatch):
    """The calls of ops.gemv_packed, as the T of each."""
    from gptq_gguf_toolkit_amd import ops
    calls, real = [], ops.gemv_packed

    def counted(q_type, blocks, x, row_src=None):
        calls.append(x.numel() // x.shape[-1])
        return real(q_type, blocks, x, row_src)

    monkeypatch.setattr(ops, "gemv_packed", counted)
    return calls


@torch.no_grad()
def incremental(model, ids, on_prefill=None):
    """Teacher-forced: prefill ids[:, :48], then one forward per token of ids[:, 48:] -> their [1, 16, V] logits."""
    out = model(input_ids=ids[:, :N_PROMPT], use_cache=True)
    if on_prefill:
        on_prefill()
    rows = []
    for i in range(N_PROMPT, ids.shape[1]):
        out = model(input_ids=ids[:, i:i + 1], past_key_values=out.past_key_values, use_cache=True)
        rows.append(out.logits[:, -1])
    return torch.stack(rows, 1).float()


@pytest.fixture(scope="module")
def world(gguf_model):  # noqa: F811
    """The file loaded dense and packed, the fp32 copy of the dense one, and floor = max |dense fp16 incremental - fp32 full
    forward| over the 16 x V logits of the teacher-forced run: torch's own 16-bit noise on this model."""
    from gptq_gguf_toolkit_amd import gguf_loader
    m = gguf_model
    dense = gguf_loader.load_into_model(load_hf(m["hf"]), m["gguf"])
    packed = gguf_loader.load_into_model(load_hf(m["hf"]), m["gguf"], packed=True)
    fp32 = copy.deepcopy(dense).float()
    ids = m["ids"][0].cuda()
    assert ids.shape == (1, N_PROMPT + N_NEW)
    with torch.no_grad():
        ref = fp32(ids).logits[:, N_PROMPT:]
    floor = float((incremental(dense, ids) - ref).abs().max())
    return dict(m, dense=dense, packed=packed, fp32=fp32, ids0=ids, ref=ref, floor=floor)


def test_teacher_forced_decode_stays_within_the_16_bit_noise_of_the_dense_model(world, gemv_calls):
    """max |packed incremental - fp32 reference| <= 2 floor: the packed path shares the dense path's roundings and differs in
    fp32 summation order only, but two independently rounded 16-bit runs can land on opposite sides of the reference."""
    before = []
    got = incremental(world["packed"], world["ids0"], on_prefill=lambda: before.append(len(gemv_calls)))
    err = float((got - world["ref"]).abs().max())
    vs_dense = float((got - incremental(world["dense"], world["ids0"])).abs().max())
    print(f"teacher-forced decode, 16 x 512 logits: floor (dense fp16 incremental against fp32) {world['floor']!r}, packed against "
          f"fp32 {err!r}, packed against dense {vs_dense!r}, max |logit| {float(world['ref'].abs().max())!r}")
    assert before == [0]                                       # the prefill of 48 tokens is the tile kernel's
    assert gemv_calls == [1] * (N_LINEARS * N_NEW)            # every Linear of every one-token step
    assert world["floor"] > 0 and bool(torch.isfinite(got).all())
    assert err <= 2 * world["floor"]


def test_greedy_on_the_packed_model(world, gemv_calls):
    from gptq_gguf_toolkit_amd.generate import greedy
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    model, prompt = world["packed"], world["ids0"][:, :N_PROMPT]
    ids, logits = greedy(model, prompt, N_NEW, return_logits=True)
    assert ids.shape == (1, N_PROMPT + N_NEW) and logits.shape == (1, N_NEW, 512) and torch.equal(ids[:, :N_PROMPT], prompt)
    assert torch.equal(ids[:, N_PROMPT:], logits.argmax(-1)) and bool(torch.isfinite(logits).all())
    assert gemv_calls == [1] * (N_LINEARS * (N_NEW - 1))       # the first new token is the prefill's
    # the routing off: the tile kernel at T = 1, no GEMV call, and logits within the same 2 floor of the fp32 model on the
    # sequence this run produced (no token equality between the paths: this model's top-2 margins go down to 0.001)
    del gemv_calls[:]
    mods = [mod for mod in model.modules() if isinstance(mod, PackedLinear)]
    assert len(mods) == N_LINEARS
    try:
        for mod in mods:
            mod.gemv_max_t = 0
        ids0, logits0 = greedy(model, prompt, N_NEW, return_logits=True)
    finally:
        for mod in mods:
            del mod.gemv_max_t
    assert gemv_calls == [] and PackedLinear.gemv_max_t > 0
    assert torch.equal(ids0[:, N_PROMPT:], logits0.argmax(-1))
    with torch.no_grad():
        ref0 = world["fp32"](ids0).logits[:, N_PROMPT - 1:-1]
        ref = world["fp32"](ids).logits[:, N_PROMPT - 1:-1]
    err0, err = float((logits0.float() - ref0).abs().max()), float((logits.float() - ref).abs().max())
    print(f"greedy, 16 x 512 logits against the fp32 model on the produced sequence: tile kernel {err0!r}, GEMV {err!r}, "
          f"floor {world['floor']!r}; {int((ids0 != ids).sum())} of 16 tokens differ between the two")
    assert err0 <= 2 * world["floor"]
    assert err <= 2 * world["floor"]


def test_generate_command_line(world):
    from gptq_gguf_toolkit_amd import generate, ppleval
    out = world["tmp"] / "gen.json"
    argv = ["--model_name_or_path", world["hf"], "--gguf", world["gguf"], "--packed", "--prompt_ids", world["ids_pt"],
            "--max_new_tokens", "8", "--dtype", "float16", "--attn_implementation", "eager", "--output_file", str(out)]
    with redirect_stdout(io.StringIO()):
        generate.main(argv)
    res = json.loads(out.read_text())
    assert res["gguf"] == world["gguf"] and res["packed"] is True and len(res["prompts"]) == len(world["ids"]) == 3
    args = generate.parse_args(argv)
    model = ppleval.apply_weights(ppleval.load_hf_model(args, torch.device("cuda")), args)
    for rec, ids in zip(res["prompts"], world["ids"]):
        assert set(rec) == {"prompt_tokens", "new_ids", "prefill_s", "decode_s", "decode_tokens_per_s"}
        assert rec["prompt_tokens"] == 64 and len(rec["new_ids"]) == 8 and all(0 <= i < 512 for i in rec["new_ids"])
        assert rec["prefill_s"] > 0 and rec["decode_s"] > 0 and rec["decode_tokens_per_s"] == pytest.approx(7 / rec["decode_s"])
        assert rec["new_ids"] == generate.greedy(model, ids.cuda(), 8)[0, 64:].tolist()
