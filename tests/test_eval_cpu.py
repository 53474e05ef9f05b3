"""Scoring a model, host side (no GPU): the three gq_eval_* symbols and their argument checks, ops.eval_* refusing CPU
tensors, metrics.py's host logic against the reference's own three floats (fixture G17, tests/golden/make_golden_eval.py)
with the kernels replaced by fp64 torch expressions, ppleval's argument rules and level database reader, quant.py's
--eval_perplexity / --eval_data."""
import ctypes
import os
import re

import pytest

from conftest import ROOT, load_golden

torch = pytest.importorskip("torch")
F = torch.nn.functional


# ------------------------------------------------------------------------------------------------ the C ABI
def test_eval_symbols_are_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf.h")).read()
    declared = set(re.findall(r"\b(gq_[a-z0-9_]+)\s*\(", hdr))
    L = _cabi.lib()
    for sym in ("gq_eval_nll", "gq_eval_kl", "gq_eval_kl_sparse"):
        assert sym in declared and sym in _cabi.EXPORTS and hasattr(L, sym), sym
        assert getattr(L, sym).argtypes, f"{sym} has no argtypes"
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6
    assert len(_cabi.EXPORTS) == 48 and "(48 symbols)" in open(os.path.join(ROOT, "README.md")).read()


def test_eval_argument_checks_need_no_device():
    """Every refusal comes before the first HIP call: a negative status and a message that names the argument."""
    from gptq_gguf_toolkit_amd import _cabi
    L, p, nul = _cabi.lib(), ctypes.c_void_p(256), ctypes.c_void_p(0)  # p: any non-NULL address, never dereferenced

    def refused(rc, status, word):
        msg = L.gq_last_error().decode()
        assert rc == status and word in msg, (rc, msg)

    # null pointers (GQ_E_NULL = -6)
    refused(L.gq_eval_nll(nul, 1, 4, 512, 512, p, -100, p, nul, nul), -6, "logits")
    refused(L.gq_eval_nll(p, 1, 4, 512, 512, nul, -100, p, nul, nul), -6, "labels")
    refused(L.gq_eval_nll(p, 1, 4, 512, 512, p, -100, nul, nul, nul), -6, "nll")
    refused(L.gq_eval_kl(p, 1, nul, 1, 4, 512, 512, 512, p, nul), -6, "target")
    refused(L.gq_eval_kl(p, 1, p, 1, 4, 512, 512, 512, nul, nul), -6, "kl")
    refused(L.gq_eval_kl_sparse(p, 1, 4, 512, 512, nul, 1, p, 32, p, nul), -6, "target_vals")
    refused(L.gq_eval_kl_sparse(p, 1, 4, 512, 512, p, 1, nul, 32, p, nul), -6, "target_ids")
    # V <= 0, ld < V (GQ_E_BAD_SHAPE = -2)
    refused(L.gq_eval_nll(p, 1, 4, 0, 512, p, -100, p, nul, nul), -2, "V=0")
    refused(L.gq_eval_kl(p, 1, p, 1, 4, -3, 512, 512, p, nul), -2, "V=-3")
    refused(L.gq_eval_kl_sparse(p, 1, 4, 0, 512, p, 1, p, 32, p, nul), -2, "V=0")
    refused(L.gq_eval_nll(p, 1, 4, 512, 511, p, -100, p, nul, nul), -2, "ld=511")
    refused(L.gq_eval_kl(p, 1, p, 1, 4, 512, 512, 100, p, nul), -2, "ld_target=100")
    # unknown dtype (GQ_E_BAD_TYPE = -1)
    refused(L.gq_eval_nll(p, 3, 4, 512, 512, p, -100, p, nul, nul), -1, "dtype 3")
    refused(L.gq_eval_kl(p, 1, p, 9, 4, 512, 512, 512, p, nul), -1, "target_dtype 9")
    refused(L.gq_eval_kl_sparse(p, -1, 4, 512, 512, p, 1, p, 32, p, nul), -1, "dtype -1")
    # K
    refused(L.gq_eval_kl_sparse(p, 1, 4, 128256, 128256, p, 1, p, 4097, p, nul), -2, "K=4097")
    refused(L.gq_eval_kl_sparse(p, 1, 4, 512, 512, p, 1, p, 0, p, nul), -2, "K=0")


def test_eval_ops_refuse_cpu_tensors():
    from gptq_gguf_toolkit_amd import GQError, ops
    x, t = torch.randn(2, 8, 32), torch.randn(2, 8, 32)
    with pytest.raises(GQError):
        ops.eval_nll(x, torch.zeros(2, 8, dtype=torch.int64))
    with pytest.raises(GQError):
        ops.eval_kl(x, t)
    with pytest.raises(GQError):
        ops.eval_kl_sparse(x, t[..., :4], torch.zeros(2, 8, 4, dtype=torch.int64))


def test_row_blocks_flatten_what_collapses_and_loop_over_the_rest():
    from gptq_gguf_toolkit_amd import ops
    x = torch.zeros(3, 10, 16)
    assert [(r, b[0][1]) for r, b in ops._row_blocks(x)] == [(30, 16)]
    assert [(r, b[0][1]) for r, b in ops._row_blocks(x[:, :-1])] == [(9, 16)] * 3       # the shifted view: one call per sequence
    assert [(r, b[0][1]) for r, b in ops._row_blocks(x[:1, :-1])] == [(9, 16)]
    assert [(r, b[0][1]) for r, b in ops._row_blocks(x[..., :12])] == [(30, 16)]        # ld > V
    assert [(r, b[0][1]) for r, b in ops._row_blocks(x[0, 0])] == [(1, 16)]
    pieces = list(ops._row_blocks(x, x.transpose(0, 1).contiguous().transpose(0, 1)))    # the second one does not collapse
    assert [r for r, _ in pieces] == [10] * 3 and all(b[1][1] == 48 for _, b in pieces)


# ------------------------------------------------------------------------------------------------ metrics.py host logic
class StubModel:
    """Returns recorded logits for recorded id rows, as a model's `.logits`; remembers what it returned."""

    def __init__(self, ids, logits):
        self.ids, self.table, self.last = ids, logits, None
        self.p = torch.nn.Parameter(torch.zeros(1, dtype=logits.dtype, device=logits.device))

    def parameters(self):
        return iter([self.p])

    def __call__(self, inputs):
        rows = [int((self.ids.to(inputs.device) == r).all(dim=1).nonzero()[0, 0]) for r in inputs]
        self.last = self.table[rows].clone()
        return type("Out", (), {"logits": self.last})()


def fp64_nll(logits, labels, ignore_index=-100, want_lse=False):
    V = logits.shape[-1]
    return F.cross_entropy(logits.double().reshape(-1, V), labels.reshape(-1), ignore_index=ignore_index,
                           reduction="none").view(labels.shape)


def fp64_kl(logits, target):
    return F.kl_div(logits.double().log_softmax(-1), target.double().log_softmax(-1), log_target=True, reduction="none").sum(-1)


def fp64_kl_sparse(logits, vals, ids):
    return fp64_kl(logits.gather(-1, ids), vals)


@pytest.fixture()
def g17():
    g = load_golden("G17_eval")
    t = lambda k: torch.from_numpy(g[k])  # noqa: E731
    return {"ids": t("ids"), "target": t("target_logits"), "quant": t("quant_logits"), "tv": t("topk_values"),
            "ti": t("topk_indices"), "ppl": float(g["ppl"]), "kl": float(g["kl"]), "sparse_kl": float(g["sparse_kl"])}


@pytest.fixture()
def patched(monkeypatch, g17):
    """metrics.py on fp64 torch expressions; every call records (was the logits argument a view of the model's output,
    did it keep the output's strides)."""
    from gptq_gguf_toolkit_amd import metrics
    model = StubModel(g17["ids"], g17["quant"])
    seen = []

    def watch(fn, shifted):
        def op(logits, *a, **k):
            out = model.last
            assert logits.untyped_storage().data_ptr() == out.untyped_storage().data_ptr(), "the logits were copied"
            assert logits.stride() == out.stride(), "the logits were re-laid-out"
            assert tuple(logits.shape) == (out.shape[0], out.shape[1] - shifted, out.shape[2])
            seen.append(tuple(logits.shape))
            return fn(logits, *a, **k)
        return op

    monkeypatch.setattr(metrics.ops, "eval_nll", watch(fp64_nll, 0))
    monkeypatch.setattr(metrics.ops, "eval_kl", watch(fp64_kl, 1))
    monkeypatch.setattr(metrics.ops, "eval_kl_sparse", watch(fp64_kl_sparse, 1))
    return metrics, model, seen


@pytest.mark.parametrize("batch_size", [1, 2, 3])  # 2: a ragged last batch (3 sequences)
def test_metrics_host_logic_reproduces_the_reference_floats(patched, g17, batch_size):
    """fp64 arithmetic on the reference's fp32 logits against the reference's fp32 run: 1e-6 relative, the reference's own
    rounding."""
    metrics, model, seen = patched
    data = [r[None] for r in g17["ids"]]
    ppl = metrics.compute_perplexity(model, data, batch_size=batch_size)
    assert seen == ([(1, 64, 512)] * 3, [(2, 64, 512), (1, 64, 512)], [(3, 64, 512)])[batch_size - 1]
    del seen[:]
    kl = metrics.compute_kl_div(model, data, [t[None] for t in g17["target"]], batch_size=batch_size)
    assert seen == ([(1, 63, 512)] * 3, [(2, 63, 512), (1, 63, 512)], [(3, 63, 512)])[batch_size - 1]
    print(f"batch {batch_size}: ppl {ppl!r} vs {g17['ppl']!r} rel {abs(ppl / g17['ppl'] - 1):.2e}; "
          f"kl {kl!r} vs {g17['kl']!r} rel {abs(kl / g17['kl'] - 1):.2e}")
    assert abs(ppl / g17["ppl"] - 1) <= 1e-6
    assert abs(kl / g17["kl"] - 1) <= 1e-6
    rows = metrics.nll_rows(model, data, batch_size=batch_size)
    assert rows.shape == (3 * 63,) and abs(float(rows.double().mean().exp()) / ppl - 1) < 1e-12


def test_sparse_metric_and_target_collection(patched, g17):
    metrics, model, seen = patched
    data = [r[None] for r in g17["ids"]]
    pairs = [(v[None], i[None]) for v, i in zip(g17["tv"], g17["ti"])]
    skl = metrics.compute_sparse_kl_div(model, data, pairs)
    print(f"sparse kl {skl!r} vs {g17['sparse_kl']!r} rel {abs(skl / g17['sparse_kl'] - 1):.2e}")
    assert seen == [(1, 63, 512)] * 3 and abs(skl / g17["sparse_kl"] - 1) <= 1e-6
    target = StubModel(g17["ids"], g17["target"])
    dense = metrics.collect_target_logits(target, data)
    assert len(dense) == 3 and all(torch.equal(d[0], t) for d, t in zip(dense, g17["target"]))
    tk = metrics.collect_target_logits(target, data, topk=32)
    for (v, i), gv, gi in zip(tk, g17["tv"], g17["ti"]):  # (values, indices), in that order
        assert v.dtype == torch.float32 and i.dtype == torch.int64 and torch.equal(v[0], gv) and torch.equal(i[0], gi)


# ------------------------------------------------------------------------------------------------ ppleval
def test_ppleval_argument_rules(tmp_path, capsys):
    from gptq_gguf_toolkit_amd import ppleval
    pt = tmp_path / "ids.pt"
    torch.save([torch.zeros(1, 8, dtype=torch.int64)], str(pt))
    base = ["--model_name_or_path", "m", "--output_file", str(tmp_path / "o.json")]
    a = ppleval.parse_args(base + ["--eval_datasets", str(pt), "--gguf", "m.gguf", "--kl_against", "gguf:t.gguf"])
    assert (a.gguf, a.kl_against, a.quant_default_level, a.eval_batch_size, a.eval_tokens, a.dtype) == \
        ("m.gguf", "gguf:t.gguf", 0, 1, 524288, "float16")
    with pytest.raises(SystemExit):
        ppleval.parse_args(base + ["--eval_datasets", str(pt), "--gguf", "m.gguf", "--quant_weights_path", "db"])
    assert "mutually exclusive" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        ppleval.parse_args(base + ["--eval_datasets", "wikitext2"])
    err = capsys.readouterr().err
    assert "must be a .pt file of token-id tensors (got 'wikitext2'); dataset downloads are not part of this package" in err
    with pytest.raises(SystemExit):
        ppleval.parse_args(base + ["--eval_datasets", str(pt), "--kl_against", "llama"])
    from gptq_gguf_toolkit_amd import metrics
    with pytest.raises(ValueError, match="dataset downloads are not part of this package"):
        metrics.load_eval_data("c4", 1024, 8)
    assert [tuple(s.shape) for s in metrics.load_eval_data(str(pt), 16, 4)] == [(1, 4)]


def test_load_compressed_weights_reads_both_file_name_forms(tmp_path):
    from gptq_gguf_toolkit_amd import level_db, ppleval
    names = ["model.layers.0.q_proj", "model.layers.0.down_proj", "model.layers.1.q_proj"]

    def model():
        m = torch.nn.Module()
        m.model = torch.nn.Module()
        m.model.layers = torch.nn.ModuleList()
        for _ in range(2):
            blk = torch.nn.Module()
            blk.q_proj, blk.down_proj = torch.nn.Linear(8, 4, bias=False), torch.nn.Linear(4, 8, bias=False)
            m.model.layers.append(blk)
        return m.half()

    gen = torch.Generator().manual_seed(3)
    w = {(n, lv): torch.randn(*((4, 8) if "q_proj" in n else (8, 4)), generator=gen) for n in names for lv in (0, 3, 4)}
    db = tmp_path / "db"
    for n in names:
        (db / n).mkdir(parents=True)
        torch.save(w[n, 0], db / n / "0.pth")            # the reference's form
        torch.save(w[n, 3], db / n / "3-Q3_K.pth")       # the splitter's HF side
        torch.save(w[n, 4], db / n / "4.5-Q4_K.pth")     # ... with --exact
    (db / "manifest.json").write_text("{}")              # files next to the layer directories are not layers

    m = ppleval.load_compressed_weights(model(), str(db))  # default level 0 -> every directory
    for n in names:
        got = m.get_submodule(n).weight
        assert got.dtype == torch.float16 and torch.equal(got, w[n, 0].half())
    m = ppleval.load_compressed_weights(model(), str(db), default_level=3)
    assert all(torch.equal(m.get_submodule(n).weight, w[n, 3].half()) for n in names)

    cfg = tmp_path / "cfg.txt"
    cfg.write_text("model.layers.0.q_proj: 3\nmodel.layers.1.q_proj: 4.5-Q4_K\n")
    fresh = model()
    before = fresh.get_submodule(names[1]).weight.clone()
    m = ppleval.load_compressed_weights(fresh, str(db), str(cfg))
    assert torch.equal(m.get_submodule(names[0]).weight, w[names[0], 3].half())
    assert torch.equal(m.get_submodule(names[2]).weight, w[names[2], 4].half())
    assert torch.equal(m.get_submodule(names[1]).weight, before)  # a config loads the listed layers only
    assert os.path.basename(level_db.find_level_file(str(db / names[0]), "4.5")) == "4.5-Q4_K.pth"
    assert os.path.basename(level_db.find_level_file(str(db / names[0]), " 0 ")) == "0.pth"
    with pytest.raises(FileNotFoundError):
        level_db.find_level_file(str(db / names[0]), 5)
    torch.save(w[names[0], 3], db / names[0] / "3-Q3_K_S.pth")
    with pytest.raises(FileNotFoundError):  # two candidates: the number alone no longer picks one
        level_db.find_level_file(str(db / names[0]), 3)
    torch.save(torch.zeros(2, 2), db / names[1] / "7.pth")
    with pytest.raises(ValueError, match="shape"):
        ppleval.load_compressed_weights(model(), str(db), default_level=7)


# ------------------------------------------------------------------------------------------------ quant.py
QUANT_ARGS = ["--model_name_or_path", "m", "--quantizable_modules", "x", "--pre_block_modules", "a", "--block_modules", "b",
              "--calibration_data", "c.pt", "--save_dir", "s"]


def test_quant_eval_perplexity_needs_eval_data(tmp_path):
    from gptq_gguf_toolkit_amd import quant
    with pytest.raises(SystemExit) as e:
        quant.main(QUANT_ARGS + ["--eval_perplexity"])
    assert str(e.value) == ("--eval_perplexity is not available in this package (WikiText-2 needs a dataset download); "
                            "run the quantization without it and evaluate the saved model separately")
    a = quant.parse_args(QUANT_ARGS + ["--eval_perplexity", "--eval_data", "x.pt"])
    assert a.eval_perplexity and a.eval_data == "x.pt" and a.eval_sequence_length == 4096
    assert quant.parse_args(QUANT_ARGS).eval_data is None
    with pytest.raises(SystemExit, match="must be a .pt file"):  # a missing file is refused before any work too
        quant.main(QUANT_ARGS + ["--eval_perplexity", "--eval_data", str(tmp_path / "missing.pt")])
