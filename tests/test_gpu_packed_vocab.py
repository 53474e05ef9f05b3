"""The vocabulary ends of a packed model on the GPU: ops.embed_packed against the dense decode, load_into_model(packed="all")
on the small quantized Llama of tests/test_gpu_eval.py (hidden 256, vocab 512, embed_tokens and lm_head Q6_K), a file without
output.weight, generate.sample and its command line, ppleval --packed_vocab."""
import copy
import io
import json
import math
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

import sample_oracle as so
from conftest import ROOT
from test_gpu_eval import gguf_model, load_hf, run_ppleval  # noqa: F401  (gguf_model: the fixture that builds the .gguf)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

N_PROMPT, N_NEW, N_LINEARS = 48, 16, 14
TYPES = (10, 11, 12, 13, 14, 8)


@pytest.mark.parametrize("q_type", TYPES)
def test_embed_packed_is_the_dense_decode_gathered(q_type):
    """Random block bytes (NaNs among the decoded values: compared as bit patterns)."""
    from gptq_gguf_toolkit_amd import ops
    V = 40
    bs, ts = ops.block_geometry(q_type)
    g = torch.Generator().manual_seed(q_type)
    for C in (256, 512):
        blocks = torch.randint(0, 256, (V, C // bs * ts), dtype=torch.uint8, generator=g).cuda()
        for dtype in (torch.float16, torch.bfloat16):
            dense = ops.dequantize_blocks(q_type, blocks, dtype)
            for ids in (torch.tensor([V - 1]), torch.cat([torch.tensor([0, V - 1, 0, 7, 7]), torch.randint(0, V, (12,), generator=g)]),
                        torch.tensor([[0, V - 1, 3], [3, 3, V - 1]])):
                for idt in (torch.int64, torch.int32):
                    got = ops.embed_packed(q_type, blocks, ids.to(idt).cuda(), dtype)
                    assert got.shape == (*ids.shape, C) and got.dtype == dtype
                    assert torch.equal(got.view(torch.int16), dense[ids.cuda()].view(torch.int16)), (C, dtype, tuple(ids.shape))
    assert ops.embed_packed(q_type, blocks, torch.zeros(0, 3, dtype=torch.int64).cuda()).shape == (0, 3, 512)


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
def incremental(model, ids):
    """Teacher-forced: prefill ids[:, :48], then one forward per token of ids[:, 48:] -> their [1, 16, V] logits."""
    out = model(input_ids=ids[:, :N_PROMPT], use_cache=True)
    rows = []
    for i in range(N_PROMPT, ids.shape[1]):
        out = model(input_ids=ids[:, i:i + 1], past_key_values=out.past_key_values, use_cache=True)
        rows.append(out.logits[:, -1])
    return torch.stack(rows, 1).float()


@pytest.fixture(scope="module")
def world(gguf_model):  # noqa: F811
    """The file loaded dense and with packed="all", the fp32 copy of the dense one, and floor = max |dense fp16 incremental -
    fp32 full forward| over the 16 x V teacher-forced logits: torch's own 16-bit noise on this model, measured on the dense
    model (never on the code under test)."""
    from gptq_gguf_toolkit_amd import gguf_loader
    m = gguf_model
    dense = gguf_loader.load_into_model(load_hf(m["hf"]), m["gguf"])
    packed = gguf_loader.load_into_model(load_hf(m["hf"]), m["gguf"], packed="all")
    fp32 = copy.deepcopy(dense).float()
    ids = m["ids"][0].cuda()
    with torch.no_grad():
        ref = fp32(ids).logits[:, N_PROMPT:]
    floor = float((incremental(dense, ids) - ref).abs().max())
    return dict(m, dense=dense, packed=packed, fp32=fp32, ids0=ids, ref=ref, floor=floor)


def test_packed_all_keeps_both_vocabulary_ends_packed(world, gemv_calls):
    from gptq_gguf_toolkit_amd import gguf_loader
    from gptq_gguf_toolkit_amd.packed_embedding import PackedEmbedding
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    packed, dense = world["packed"], world["dense"]
    emb, head = packed.model.embed_tokens, packed.lm_head
    assert type(emb) is PackedEmbedding and type(head) is PackedLinear and emb.q_type == head.q_type == 14
    assert emb.weight.is_meta and head.weight.is_meta and head.row_src is None
    assert emb.blocks.data_ptr() != head.blocks.data_ptr()  # the file has an output.weight of its own
    assert sum(isinstance(mod, PackedLinear) for mod in packed.modules()) == N_LINEARS + 1
    assert gguf_loader.packed_vocab_tensors(load_hf(world["hf"]), world["gguf"]) == {
        "model.embed_tokens": ("token_embd.weight", 14), "lm_head": ("output.weight", 14)}
    assert not any(k.startswith(("lm_head", "model.embed_tokens")) for k in packed.state_dict())
    ids = world["ids0"]
    assert torch.equal(emb(ids).view(torch.int16), dense.model.embed_tokens(ids).view(torch.int16))
    assert torch.equal(head.dense_weight().view(torch.int16), dense.lm_head.weight.data.view(torch.int16))
    del gemv_calls[:]
    got = incremental(packed, ids)
    assert gemv_calls == [1] * ((N_LINEARS + 1) * N_NEW)  # every Linear of every one-token step, lm_head among them
    err = float((got - world["ref"]).abs().max())
    print(f"teacher-forced decode with packed vocabulary ends, 16 x 512 logits: floor {world['floor']!r}, against fp32 {err!r}")
    assert world["floor"] > 0 and bool(torch.isfinite(got).all())
    assert err <= 2 * world["floor"]


def test_packed_true_still_leaves_both_ends_dense(world):
    from gptq_gguf_toolkit_amd import gguf_loader
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    model = gguf_loader.load_into_model(load_hf(world["hf"]), world["gguf"], packed=True)
    assert type(model.lm_head) is torch.nn.Linear and type(model.model.embed_tokens) is torch.nn.Embedding
    assert sum(isinstance(mod, PackedLinear) for mod in model.modules()) == N_LINEARS
    with pytest.raises(ValueError, match="packed"):
        gguf_loader.load_into_model(load_hf(world["hf"]), world["gguf"], packed="vocab")


def test_a_file_without_output_weight_shares_one_copy(world):
    import gguf_spec_writer as W
    from gptq_gguf_toolkit_amd import gguf_loader
    from gptq_gguf_toolkit_amd.gguf_writer import parse_gguf
    from gptq_gguf_toolkit_amd.packed_embedding import PackedEmbedding
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    kv, tensors, buf = parse_gguf(world["gguf"])
    kind, tname = {v: k for k, v in W.VT.items()}, {v: k for k, v in W.GGML.items()}
    kvs = [(k, ("arr", kind[t[1]]) if len(t) == 2 else kind[t[0]], v) for k, (v, t) in kv.items()]
    kept = [(n, shape, tname[gt], bytes(buf[off:off + nb])) for n, shape, gt, off, nb in tensors if n != "output.weight"]
    assert len(kept) == len(tensors) - 1
    path = world["tmp"] / "tied.gguf"
    path.write_bytes(W.serialise(kvs, kept))

    def tied():
        model = load_hf(world["hf"])
        model.lm_head.weight = model.model.embed_tokens.weight
        return model

    assert gguf_loader.packed_vocab_tensors(tied(), str(path)) == {
        "model.embed_tokens": ("token_embd.weight", 14), "lm_head": ("token_embd.weight", 14)}
    model = gguf_loader.load_into_model(tied(), str(path), packed="all")
    emb, head = model.model.embed_tokens, model.lm_head
    assert type(emb) is PackedEmbedding and type(head) is PackedLinear
    assert emb.blocks.data_ptr() == head.blocks.data_ptr()
    dense = gguf_loader.load_into_model(tied(), str(path))
    assert dense.lm_head.weight.data_ptr() == dense.model.embed_tokens.weight.data_ptr()
    ids = world["ids0"]
    with torch.no_grad():
        got, want = model(ids).logits.float(), dense(ids).logits.float()
        ref = copy.deepcopy(dense).float()(ids).logits
    floor, err = float((want - ref).abs().max()), float((got - ref).abs().max())
    print(f"tied file, 64 x 512 logits against fp32: dense {floor!r}, packed {err!r}")
    assert err <= 2 * floor


def test_sample_on_the_packed_model(world):
    from gptq_gguf_toolkit_amd.generate import sample
    model, prompt = world["packed"], world["ids0"][:, :N_PROMPT]
    ids, logits = sample(model, prompt, N_NEW, temperature=0.0, return_logits=True)
    assert ids.shape == (1, N_PROMPT + N_NEW) and logits.shape == (1, N_NEW, 512) and torch.equal(ids[:, :N_PROMPT], prompt)
    z = logits[0].float().cpu().numpy()
    assert ids[0, N_PROMPT:].tolist() == [so.sample(z[i], 0.0, 40, 1.0, 0.0) for i in range(N_NEW)]

    def run(seed):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        return sample(model, prompt.repeat(2, 1), N_NEW, temperature=2.0, top_k=50, top_p=0.95, generator=g)

    a, b, c = run(5), run(5), run(6)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert a.shape == (2, N_PROMPT + N_NEW) and bool(((a >= 0) & (a < 512)).all())
    # a row stops at its eos; the batch is cut where the last row stops
    tm = {}
    eos = int(a[0, N_PROMPT + 2])
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    d = sample(model, prompt.repeat(2, 1), N_NEW, temperature=2.0, top_k=50, top_p=0.95, generator=g, eos_token_id=eos,
               pad_token_id=0, eos_poll=4, timings=tm)
    new = d[:, N_PROMPT:]
    first = [row.tolist().index(eos) if eos in row.tolist() else None for row in new]
    assert first[0] is not None and first[0] <= 2 and torch.equal(new[0, :first[0] + 1], a[0, N_PROMPT:N_PROMPT + first[0] + 1])
    assert bool((new[0, first[0] + 1:] == 0).all())
    assert tm["stopped_at_eos"] == all(f is not None for f in first)
    if tm["stopped_at_eos"]:
        assert new.shape[1] == max(first) + 1
    else:
        assert new.shape[1] == N_NEW


def test_generate_command_line_samples(world):
    from gptq_gguf_toolkit_amd import generate
    base = ["--model_name_or_path", world["hf"], "--gguf", world["gguf"], "--packed", "--packed_vocab", "--prompt_ids",
            world["ids_pt"], "--max_new_tokens", "8", "--dtype", "float16", "--attn_implementation", "eager"]
    out = world["tmp"] / "gen_s.json"
    with redirect_stdout(io.StringIO()):
        generate.main(base + ["--output_file", str(out), "--do_sample", "--seed", "3", "--temperature", "1.5", "--top_k", "20"])
        res = json.loads(out.read_text())
        generate.main(base + ["--output_file", str(out), "--do_sample", "--seed", "3", "--temperature", "1.5", "--top_k", "20"])
    assert [r["new_ids"] for r in res["prompts"]] == [r["new_ids"] for r in json.loads(out.read_text())["prompts"]]  # the seed
    for rec in res["prompts"]:
        assert set(rec) == {"prompt_tokens", "new_ids", "prefill_s", "decode_s", "decode_tokens_per_s", "sampled", "seed",
                            "stopped_at_eos"}
        assert rec["sampled"] is True and rec["seed"] == 3 and rec["stopped_at_eos"] is False
        assert len(rec["new_ids"]) == 8 and all(0 <= i < 512 for i in rec["new_ids"])
    out_g = world["tmp"] / "gen_g.json"
    with redirect_stdout(io.StringIO()):
        generate.main(base + ["--output_file", str(out_g)])
    res_g = json.loads(out_g.read_text())
    assert set(res_g) == {"model_name_or_path", "gguf", "packed", "quant_weights_path", "quant_config_path", "max_new_tokens",
                          "prompts"}
    for rec in res_g["prompts"]:
        assert set(rec) == {"prompt_tokens", "new_ids", "prefill_s", "decode_s", "decode_tokens_per_s"}


def test_ppleval_packed_vocab(world):
    """ln ppl is the mean of lse(x) - x[label] over the rows, and that is 2-Lipschitz in max |x|: two models whose logits
    differ by at most e from a reference differ from its ln ppl by at most 2 e.  The packed model's logits are held to 2
    floor of the fp32 copy (the rule above), so |ln ppl(packed) - ln ppl(fp32)| <= 4 floor, with the floor measured on the
    dense fp16 model over the same 3 x 64 tokens."""
    res, scored = run_ppleval(world, "pv", "--gguf", world["gguf"], "--packed", "--packed_vocab")
    from gptq_gguf_toolkit_amd.packed_embedding import PackedEmbedding
    assert type(scored.model.embed_tokens) is PackedEmbedding
    ppl = res["perplexity_results"][world["ids_pt"]]
    data = torch.cat(world["ids"]).cuda()
    with torch.no_grad():
        ref = world["fp32"](data).logits
        floor = float((world["dense"](data).logits.float() - ref).abs().max())
        nll = torch.nn.functional.cross_entropy(ref[:, :-1].reshape(-1, 512).double(), data[:, 1:].reshape(-1))
    print(f"ppleval --packed --packed_vocab: {ppl!r}; fp32 model {math.exp(float(nll))!r}; floor {floor!r}")
    assert np.isfinite(ppl) and abs(math.log(ppl) - float(nll)) <= 4 * floor
