"""Sampled generation, host side (no GPU): the additive header include/gptq_gguf_sample.h and its binding, every refusal of
gq_sample_logits -- made before the first HIP call, so host pointers do --, the Python layers' refusals, PackedEmbedding's
size rule, generate's new flags, and generate.sample on the fp32 CPU tiny Llama with ops.sample_logits replaced by the fp64
oracle of its contract (tests/sample_oracle.py): the cache, EOS and polling plumbing."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import sample_oracle as so
from conftest import ROOT

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

P = 256  # any 16-byte aligned address, never dereferenced
F32, F16, BF16 = 0, 1, 2
BAD_TYPE, BAD_SHAPE, NULL = -1, -2, -6


def _msg(L):
    return L.gq_last_error().decode()


def test_sample_header_symbol_is_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi, ops
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_sample.h")).read()
    declared = set(re.findall(r"^int (gq_[a-z0-9_]+)\s*\(", hdr, re.M))
    L = _cabi.lib()
    assert declared == set(_cabi.EXPORTS_SAMPLE) == {"gq_sample_logits"}
    assert hasattr(ctypes.CDLL(_cabi.SO_PATH), "gq_sample_logits") and len(L.gq_sample_logits.argtypes) == 11
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6 and len(_cabi.EXPORTS) == 48  # additive: the version stays
    assert int(re.search(r"#define GQ_SAMPLE_MAX_K (\d+)", hdr).group(1)) == _cabi.SAMPLE_MAX_K == ops.SAMPLE_MAX_K == 1024
    for word in ("index ascending", "Deterministic", "unbounded nucleus", "temperature, then top-k, then top-p"):
        assert word in hdr, word
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "gq_sample_logits" in text, doc
    assert "(48 symbols)" in open(os.path.join(ROOT, "README.md")).read()
    src = open(os.path.join(ROOT, "gptq-gguf-toolkit_amd", "csrc", "Makefile")).read()
    assert "sample/gq_sample.hip" in src and "gptq_gguf_sample.h" in src


def test_sample_logits_refusals_need_no_device():
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()

    def call(logits=P, dtype=F16, B=2, V=100, ld=100, top_k=40, top_p=0.9, temperature=1.0, u=P, ids=P):
        return L.gq_sample_logits(logits, dtype, B, V, ld, top_k, top_p, temperature, u, ids, None)

    def refused(status, word, **kw):
        rc = call(**kw)
        assert rc == status and word in _msg(L) and "gq_sample_logits" in _msg(L), (kw, rc, _msg(L))

    refused(BAD_TYPE, "dtype 3", dtype=3)
    refused(BAD_TYPE, "dtype -1", dtype=-1)
    refused(NULL, "logits is NULL", logits=None)
    refused(NULL, "ids is NULL", ids=None)
    refused(NULL, "u is NULL", u=None)
    refused(NULL, "u is NULL", u=None, temperature=1e-3)
    refused(BAD_SHAPE, "B=0", B=0)
    refused(BAD_SHAPE, "B=-1", B=-1)
    refused(BAD_SHAPE, "V=0", V=0, ld=0)
    refused(BAD_SHAPE, "ld=99", ld=99)
    refused(BAD_SHAPE, "top_k=1025", top_k=1025)
    refused(BAD_SHAPE, "top_k=0", top_k=0)            # "no top-k" is not built and nothing is substituted
    refused(BAD_SHAPE, "top_k=-1", top_k=-1)
    refused(BAD_SHAPE, "top_p=0", top_p=0.0)
    refused(BAD_SHAPE, "top_p=1.5", top_p=1.5)
    refused(BAD_SHAPE, "top_p=-0.5", top_p=-0.5)
    refused(BAD_SHAPE, "top_p=nan", top_p=float("nan"))
    refused(BAD_SHAPE, "temperature=-1", temperature=-1.0)
    refused(BAD_SHAPE, "temperature=nan", temperature=float("nan"))
    refused(BAD_SHAPE, "logits is not aligned", logits=P + 1)
    refused(BAD_SHAPE, "logits is not aligned", logits=P + 2, dtype=F32)
    refused(BAD_SHAPE, "u not 4-byte aligned", u=P + 2)
    refused(BAD_SHAPE, "ids not 8-byte aligned", ids=P + 4)
    # the order: dtype, NULL logits / ids, B, V, ld, top_k, top_p, temperature, NULL u, alignments
    refused(BAD_TYPE, "dtype 3", dtype=3, logits=None, top_k=0)
    refused(NULL, "logits is NULL", logits=None, top_k=0)
    refused(BAD_SHAPE, "ld=99", ld=99, top_k=0)
    refused(BAD_SHAPE, "top_k=0", top_k=0, top_p=2.0)
    refused(BAD_SHAPE, "top_p=2", top_p=2.0, temperature=-1.0)
    refused(BAD_SHAPE, "temperature=-1", temperature=-1.0, u=None)
    # top_k = 1024 and top_p = 1 are the last values that pass their rules: the refusal is a LATER check's
    refused(NULL, "u is NULL", top_k=1024, top_p=1.0, u=None)
    refused(BAD_SHAPE, "ids not 8-byte aligned", top_k=1024, top_p=1.0, ids=P + 4)
    refused(BAD_SHAPE, "ids not 8-byte aligned", top_k=1, temperature=0.0, u=None, ids=P + 4)  # (u may be NULL at 0)
    refused(BAD_SHAPE, "u not 4-byte aligned", top_k=1024, ld=103, u=P + 1)


def test_ops_refuse_cpu_tensors_and_bad_id_dtypes(monkeypatch):
    from gptq_gguf_toolkit_amd import _cabi, ops
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.sample_logits(torch.zeros(2, 8), torch.zeros(2), 4)
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.embed_packed(12, torch.zeros(4, 144, dtype=torch.uint8), torch.zeros(3, dtype=torch.int64))
    # the shape and dtype rules, with the device check out of the way
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)
    blocks = torch.zeros(4, 144, dtype=torch.uint8)
    for ids in (torch.zeros(3, dtype=torch.int16), torch.zeros(3, dtype=torch.uint8), torch.zeros(3), torch.zeros(3, dtype=torch.bool)):
        with pytest.raises(_cabi.GQError, match="int32 or int64"):
            ops.embed_packed(12, blocks, ids)
    for bad in (torch.zeros(4, 143, dtype=torch.uint8), torch.zeros(4, 144, dtype=torch.int8), torch.zeros(4 * 144, dtype=torch.uint8)):
        with pytest.raises(_cabi.GQError, match="packed blocks"):
            ops.embed_packed(12, bad, torch.zeros(3, dtype=torch.int64))
    x, u = torch.zeros(2, 8), torch.zeros(2)
    for kw, word in ((dict(top_k=0), "top_k=0"), (dict(top_k=1025), "top_k=1025"), (dict(top_k=4, u=None), "u is None"),
                     (dict(top_k=4, u=torch.zeros(3)), "u must be"), (dict(top_k=4, u=torch.zeros(2, dtype=torch.float64)), "u must be"),
                     (dict(top_k=4, logits=torch.zeros(2, 8, dtype=torch.int64)), "logits must be"),
                     (dict(top_k=4, logits=torch.zeros(8)), "logits must be"),
                     (dict(top_k=4, logits=torch.zeros(2, 16)[:, ::2]), "logits must be"),
                     (dict(top_k=4, logits=torch.zeros(1, 8).expand(2, 8)), "rows overlap")):
        args = dict(logits=x, u=u)
        args.update(kw)
        with pytest.raises(_cabi.GQError, match=word):
            ops.sample_logits(args.pop("logits"), args.pop("u"), **args)


def test_packed_embedding_size_rule_dense_level_and_no_level():
    from gptq_gguf_toolkit_amd._cabi import GQError
    from gptq_gguf_toolkit_amd.packed_embedding import PackedEmbedding, replace_embedding
    emb = PackedEmbedding(10, 256)
    assert emb.weight.is_meta and tuple(emb.weight.shape) == (10, 256) and emb.dtype == torch.float16
    assert list(emb.parameters()) == [] and emb.state_dict() == {}
    with pytest.raises(GQError, match="no level"):
        emb(torch.zeros(2, dtype=torch.int64))
    emb.set_level(torch.zeros(10, 210, dtype=torch.uint8), 14)      # Q6_K: 210 bytes per 256 values
    emb.set_level(torch.zeros(10 * 144, dtype=torch.uint8), 12)     # any view of exactly the bytes
    emb.set_level(torch.zeros(10, 8 * 34, dtype=torch.uint8), 8)    # Q8_0: 8 blocks of 34 bytes
    for blocks, q in ((torch.zeros(10, 209, dtype=torch.uint8), 14), (torch.zeros(9, 210, dtype=torch.uint8), 14),
                      (torch.zeros(10, 210, dtype=torch.int8), 14), (torch.zeros(10, 210, dtype=torch.uint8), 12)):
        with pytest.raises(GQError, match="set_level"):
            emb.set_level(blocks, q)
    with pytest.raises(GQError, match="set_level"):
        PackedEmbedding(10, 128).set_level(torch.zeros(10, 4 * 34, dtype=torch.uint8), 8)  # embedding_dim % 256
    for bad in (torch.zeros(10, 256), torch.zeros(256, 10, dtype=torch.float16)):
        with pytest.raises(GQError, match="dense level"):
            emb.set_level(bad, None)
    table = torch.arange(10 * 256, dtype=torch.float32).reshape(10, 256).to(torch.float16)
    emb.set_level(table, None)                                      # a dense level: F.embedding on the stored tensor
    ids = torch.tensor([[0, 9], [3, 3]])
    assert torch.equal(emb(ids), torch.nn.functional.embedding(ids, table))
    with pytest.raises(TypeError):
        PackedEmbedding(10, 256, torch.int8)
    holder = torch.nn.Sequential(torch.nn.Embedding(10, 256), torch.nn.Linear(256, 4))
    got = replace_embedding(holder, "0")
    assert holder[0] is got and type(got) is PackedEmbedding and got.dtype == torch.float32
    with pytest.raises(TypeError):
        replace_embedding(holder, "1")


def test_new_flags_parse(capsys):
    from gptq_gguf_toolkit_amd import generate, ppleval
    base = ["--model_name_or_path", "m", "--prompt_ids", "ids.pt", "--max_new_tokens", "5", "--output_file", "o.json"]
    a = generate.parse_args(base)
    assert (a.do_sample, a.temperature, a.top_k, a.top_p, a.seed, a.eos_token_id, a.packed_vocab) == (False, 1.0, 40, 1.0, 0, None, False)
    a = generate.parse_args(base + ["--gguf", "f", "--packed", "--packed_vocab", "--do_sample", "--temperature", "0.7", "--top_k",
                                    "1024", "--top_p", "0.9", "--seed", "3", "--eos_token_id", "2", "7"])
    assert (a.do_sample, a.temperature, a.top_k, a.top_p, a.seed, a.eos_token_id, a.packed_vocab) == (True, 0.7, 1024, 0.9, 3, [2, 7], True)
    for bad, word in ((["--gguf", "f", "--packed_vocab"], "--packed_vocab needs --packed"), (["--top_k", "0"], "--top_k"),
                      (["--top_k", "1025"], "--top_k"), (["--top_p", "0"], "--top_p"), (["--temperature", "-1"], "--temperature")):
        with pytest.raises(SystemExit):
            generate.parse_args(base + bad)
        assert word in capsys.readouterr().err
    here = os.path.abspath(__file__)
    pbase = ["--model_name_or_path", "m", "--eval_datasets", here, "--output_file", "o.json"]
    assert ppleval.parse_args(pbase + ["--gguf", "f", "--packed", "--packed_vocab"]).packed_vocab is True
    assert ppleval.parse_args(pbase + ["--gguf", "f", "--packed"]).packed_vocab is False
    with pytest.raises(SystemExit):
        ppleval.parse_args(pbase + ["--gguf", "f", "--packed_vocab"])
    assert "--packed_vocab needs --packed" in capsys.readouterr().err

    class Args:
        gguf, packed, packed_vocab, quant_weights_path = "f.gguf", True, True, None

    seen = []
    import gptq_gguf_toolkit_amd.gguf_loader as gl
    real = gl.load_into_model
    gl.load_into_model = lambda model, path, packed=False: seen.append(packed)
    try:
        ppleval.apply_weights(None, Args)
        Args.packed_vocab = False
        ppleval.apply_weights(None, Args)
        Args.packed = False
        ppleval.apply_weights(None, Args)
    finally:
        gl.load_into_model = real
    assert seen == ["all", True, False]


@pytest.fixture()
def oracle_sampler(monkeypatch):
    """ops.sample_logits replaced by the oracle on CPU tensors -> the list of (u, top_k, top_p, temperature) it was called with."""
    from gptq_gguf_toolkit_amd import ops
    calls = []

    def fake(logits, u, top_k, top_p=1.0, temperature=1.0):
        assert logits.dim() == 2 and (u is None) == (temperature == 0)
        calls.append((None if u is None else u.clone(), top_k, top_p, temperature))
        z = logits.float().numpy()
        return torch.tensor([so.sample(z[b], 0.0 if u is None else float(u[b]), top_k, float(np.float32(top_p)),
                                       float(np.float32(temperature))) for b in range(z.shape[0])], dtype=torch.int64)

    monkeypatch.setattr(ops, "sample_logits", fake)
    return calls


def test_sample_at_temperature_zero_is_greedy_and_keeps_one_row_of_prefill_logits(oracle_sampler, monkeypatch):
    """Samples 0 and 1 of tiny_calib(n=3, L=64, seed=29): their top-2 margins are >= 0.005 (tests/test_qgemv_cpu.py), so the
    argmax does not hang on a tie order."""
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd.generate import greedy, sample
    model = tiny_llama().eval()
    calib = tiny_calib(n=3, L=64, seed=29)
    kept = []
    real = type(model).forward

    def spy(self, *a, **kw):
        out = real(self, *a, **kw)
        kept.append((kw.get("logits_to_keep"), tuple(out.logits.shape)))
        return out

    monkeypatch.setattr(type(model), "forward", spy)
    for i in (0, 1):
        prompt = calib[i][:, :48]
        want, want_logits = greedy(model, prompt, 16, return_logits=True)
        del kept[:]
        tm = {}
        ids, logits = sample(model, prompt, 16, temperature=0.0, return_logits=True, timings=tm)
        assert torch.equal(ids, want) and logits.shape == (1, 16, 512)
        assert float((logits - want_logits).abs().max()) <= 1e-4
        assert kept[0] == (1, (1, 1, 512)) and all(k == (None, (1, 1, 512)) for k in kept[1:]) and len(kept) == 16
        assert set(tm) == {"prefill_s", "decode_s", "stopped_at_eos"} and tm["stopped_at_eos"] is False
    assert all(c[0] is None for c in oracle_sampler)  # the argmax draws nothing

    # eos = the third token that run produces: the result ends there, whatever the polling interval
    prompt = calib[0][:, :48]
    full = greedy(model, prompt, 16)[0, 48:].tolist()
    eos = full[2]
    cut = full.index(eos) + 1
    outs = []
    for poll in (1, 8, 3):
        tm = {}
        del kept[:]
        got = sample(model, prompt, 16, temperature=0.0, eos_token_id=eos, eos_poll=poll, timings=tm)
        assert got[0, 48:].tolist() == full[:cut] and tm["stopped_at_eos"] is True
        outs.append(len(kept))
    assert outs[0] == cut and outs[1] == min(16, 8) and outs[0] <= outs[2] <= outs[1]  # forwards run: polling costs steps only
    tm = {}
    got = sample(model, prompt, 2, temperature=0.0, eos_token_id=[eos, eos], timings=tm)  # (a list; max_new_tokens comes first)
    assert got[0, 48:].tolist() == full[:min(2, cut)] and tm["stopped_at_eos"] is (cut <= 2)

    # B = 2: the finished row is fed and filled with the pad id, the other row runs on
    other = greedy(model, calib[1][:, :48], 16)[0, 48:].tolist()
    both = torch.cat([prompt, calib[1][:, :48]])
    for poll in (1, 8):
        tm = {}
        got = sample(model, both, 16, temperature=0.0, eos_token_id=eos, pad_token_id=7, eos_poll=poll, timings=tm)
        stop1 = other.index(eos) + 1 if eos in other else 16
        assert got.shape == (2, 48 + max(cut, stop1))
        assert got[0, 48:].tolist() == full[:cut] + [7] * (got.shape[1] - 48 - cut)
        assert got[1, 48:48 + stop1].tolist() == other[:stop1]
        assert tm["stopped_at_eos"] is (eos in other)


def test_sample_draws_with_the_generator_and_refuses_bad_arguments(oracle_sampler):
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd.generate import sample
    model = tiny_llama().eval()
    prompt = tiny_calib(n=3, L=64, seed=29)[0][:, :48].repeat(2, 1)
    g = torch.Generator().manual_seed(11)
    a = sample(model, prompt, 6, temperature=2.0, top_k=50, top_p=0.9, generator=g)
    us = [c[0] for c in oracle_sampler]
    assert len(us) == 6 and all(u.shape == (2,) and u.dtype == torch.float32 for u in us)
    g2 = torch.Generator().manual_seed(11)
    assert all(torch.equal(u, torch.rand(2, generator=g2)) for u in us)
    assert all(c[1:] == (50, 0.9, 2.0) for c in oracle_sampler)
    assert torch.equal(a, sample(model, prompt, 6, temperature=2.0, top_k=50, top_p=0.9, generator=torch.Generator().manual_seed(11)))
    assert not torch.equal(a[0], a[1])  # two draws per step: the rows of one prompt part
    for kw in (dict(top_k=0), dict(top_k=1025), dict(top_p=0.0), dict(top_p=1.1), dict(temperature=-0.5), dict(eos_poll=0)):
        with pytest.raises(ValueError):
            sample(model, prompt, 4, **kw)
    with pytest.raises(ValueError, match="max_new_tokens"):
        sample(model, prompt, 0)
