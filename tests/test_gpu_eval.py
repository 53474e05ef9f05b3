"""-m gpu: K16, scoring on the GPU -- gq_eval_nll / gq_eval_kl / gq_eval_kl_sparse, metrics.py, ppleval, quant.py --eval_data.

The tolerance rule of every kernel comparison (error_rule below): the reference value is the torch expression in fp64 on
the same inputs; torch's OWN fp32 path (F.cross_entropy(logits.float(), reduction="none"), or the reference's KL expression
in fp32) is measured against it in the same test, and the kernel's maximum error over the test's rows must stay within
4 x that.  The hardware exp2 is a couple of ulp where libm is correctly rounded and the summation order differs; a
factor 4 over measured fp32 noise allows for both and still catches a wrong formula.  A test pools all its T (or K) cases
before it compares the two maxima: the maximum over a single row (T = 1) is one draw of the noise, not its size.
Both figures are printed (pytest -s).

Measured on an MI355X (max |error| kernel / torch fp32; the worst ratio of each kind): nll f16 V=128256 1.8e-6 / 1.3e-6
(1.41), dense KL f16 V=128256 1.0e-6 / 9.0e-7 (1.12), sparse KL 3.0e-7 / 7.4e-7 (0.41); all other cases 0.3 - 1.2
(DESIGN.md K16).  The fixed atol 4e-6 of the special-value tests compares kernel and torch fp32 DIRECTLY on two finite rows:
4 ulp of fp32 at lse ~ 12 (ulp 9.5e-7), i.e. both sides at the noise measured above."""
import io
import json
import math
import os
import re
import sys
from contextlib import redirect_stdout

import pytest

from conftest import ROOT, load_golden

torch = pytest.importorskip("torch")
F = torch.nn.functional
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
VS = (512, 32000, 50257, 128256)  # 50257 is odd: every second fp16 row starts 2-byte aligned
TS = (1, 3, 2047)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from gptq_gguf_toolkit_amd import ops as _ops
    return _ops


def nll64(logits, labels, ignore_index=-100):
    return F.cross_entropy(logits.double(), labels, ignore_index=ignore_index, reduction="none")


def nll32(logits, labels, ignore_index=-100):
    return F.cross_entropy(logits.float(), labels, ignore_index=ignore_index, reduction="none")


def kl_expr(logits, target):
    """metrics.py:70-75 of the reference, per row (before its batchmean), in the dtype it is given."""
    return F.kl_div(logits.log_softmax(dim=-1), target.log_softmax(dim=-1), log_target=True, reduction="none").sum(-1)


class Errors:
    """Pools max |x - fp64| of the kernel and of torch's fp32 path over the cases of one test."""

    def __init__(self, what):
        self.what, self.kernel, self.torch32 = what, 0.0, 0.0

    def add(self, got, ref64, t32):
        assert got.dtype == torch.float32 and got.shape == ref64.shape
        assert torch.isfinite(got).all() and torch.isfinite(ref64).all()
        self.kernel = max(self.kernel, float((got.double() - ref64).abs().max()))
        self.torch32 = max(self.torch32, float((t32.double() - ref64).abs().max()))

    def check(self):
        print(f"\n[error_rule] {self.what}: kernel {self.kernel:.3e}  torch fp32 {self.torch32:.3e}  "
              f"ratio {self.kernel / self.torch32 if self.torch32 else float('inf'):.2f}")
        assert self.kernel <= 4.0 * self.torch32, (self.what, self.kernel, self.torch32)


def make_logits(T, V, dtype, seed, ld=None):
    g = torch.Generator(device="cuda").manual_seed(seed)
    big = (torch.randn(T, ld or V, device="cuda", generator=g) * 3.0).to(dtype)
    return big[:, :V]


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_nll_against_fp64(ops, dt, V):
    e = Errors(f"nll {dt} V={V}")
    for T in TS:
        x = make_logits(T, V, DTYPES[dt], seed=V + T)
        g = torch.Generator(device="cuda").manual_seed(T)
        labels = torch.randint(0, V, (T,), device="cuda", generator=g)
        got, lse = ops.eval_nll(x, labels, want_lse=True)
        e.add(got, nll64(x, labels), nll32(x, labels))
        assert torch.equal(got, ops.eval_nll(x, labels))  # the same bits with and without lse, launch after launch
        assert float((lse.double() - x.double().logsumexp(-1)).abs().max()) <= 4 * e.torch32
        del x
    e.check()


@pytest.mark.parametrize("dt", list(DTYPES))
def test_nll_row_stride_ignore_index_and_leading_dims(ops, dt):
    V, e = 50257, Errors(f"nll {dt} ld > V, ignore_index, [B, L, V]")
    x = make_logits(6 * 37, V, DTYPES[dt], seed=3, ld=V + 24)  # ld = V + 24: rows at every 2-byte (4-byte) phase
    assert x.stride(0) == V + 24 and not x.is_contiguous()
    g = torch.Generator(device="cuda").manual_seed(4)
    labels = torch.randint(0, V, (6 * 37,), device="cuda", generator=g)
    labels[torch.rand(6 * 37, device="cuda", generator=g) < 0.3] = -100
    labels[0], labels[-1] = -100, 7
    got, lse = ops.eval_nll(x, labels, want_lse=True)
    assert bool((got[labels == -100] == 0).all()) and bool((labels == -100).sum() > 20)
    e.add(got, nll64(x, labels), nll32(x, labels))
    assert float((lse.double() - x.double().logsumexp(-1)).abs().max()) <= 4 * e.torch32  # lse of ignored rows too
    assert torch.equal(ops.eval_nll(x, labels.masked_fill(labels == -100, 5), ignore_index=5), got)
    x3, l3 = x.view(6, 37, V), labels.view(6, 37)  # one row stride: one launch
    assert torch.equal(ops.eval_nll(x3, l3), got.view(6, 37))
    sh = ops.eval_nll(x3[:, :-1], l3[:, 1:].contiguous())  # the reference's shifted view: looped over, not copied
    e.add(sh[l3[:, 1:] != -100], nll64(x3[:, :-1].reshape(-1, V), l3[:, 1:].reshape(-1))[l3[:, 1:].reshape(-1) != -100],
          nll32(x3[:, :-1].reshape(-1, V), l3[:, 1:].reshape(-1))[l3[:, 1:].reshape(-1) != -100])
    e.check()


def test_nll_special_values_follow_torch(ops):
    V = 1000
    for dt in DTYPES.values():
        x = make_logits(8, V, dt, seed=11).clone()
        labels = torch.full((8,), 5, device="cuda", dtype=torch.int64)
        inf = float("inf")
        x[1, 17] = float("nan")              # a NaN anywhere -> NaN
        x[2, 100:900] = -inf                 # -inf logits are legal
        x[3, 5] = -inf                       # the label's logit is -inf -> +inf
        x[4, :] = -inf                       # all -inf -> NaN
        x[5, 3] = inf                        # +inf -> NaN
        x[6, :] = float("nan")
        x[7, 0] = float("nan"); x[7, 1:] = -inf  # noqa: E702
        got, lse = ops.eval_nll(x, labels, want_lse=True)
        want = nll32(x, labels)
        assert torch.isnan(got[[1, 4, 5, 6, 7]]).all() and torch.isnan(want[[1, 4, 5, 6, 7]]).all(), (got, want)
        assert got[3].item() == inf == want[3].item()
        assert torch.isfinite(got[[0, 2]]).all()
        torch.testing.assert_close(got[[0, 2]], want[[0, 2]], rtol=0, atol=4e-6)
        ref_lse = x.float().logsumexp(-1)
        assert torch.isnan(lse[[1, 6, 7]]).all() and lse[4].item() == -inf == ref_lse[4].item()
        assert lse[5].item() == inf or math.isnan(lse[5].item())  # torch.logsumexp: inf; log_softmax (and the loss): NaN
        labels[2] = -100                     # an ignored row is 0 whatever it holds
        labels[6] = -100
        got = ops.eval_nll(x, labels)
        assert got[2].item() == 0.0 and got[6].item() == 0.0 and nll32(x, labels)[6].item() == 0.0


def test_nll_out_of_range_label_is_a_status_not_a_read(ops):
    from gptq_gguf_toolkit_amd import GQError
    x = make_logits(5, 512, torch.float16, seed=2)
    for bad in (512, -1, 1 << 40):
        labels = torch.tensor([1, 2, bad, 3, -100], device="cuda")
        with pytest.raises(GQError, match=r"status -2.*label lies outside \[0, V=512\)"):
            ops.eval_nll(x, labels)
    good = torch.tensor([1, 2, 511, 0, -100], device="cuda")
    assert torch.isfinite(ops.eval_nll(x, good)).all()  # the flag does not stick


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_kl_against_fp64(ops, dt, V):
    e = Errors(f"kl {dt} V={V}")
    for T in TS:
        t = make_logits(T, V, DTYPES[dt], seed=2 * V + T)
        x = (t.float() + 0.3 * make_logits(T, V, torch.float32, seed=V + 7 * T) / 3.0).to(DTYPES[dt])
        got = ops.eval_kl(x, t)
        assert bool((got > 0).all()) and torch.equal(got, ops.eval_kl(x, t))
        e.add(got, kl_expr(x.double(), t.double()), kl_expr(x.float(), t.float()))
        assert bool((ops.eval_kl(t, t) == 0).all())  # identical operands: exactly 0
        del x, t
    e.check()


def test_kl_views_strides_and_mixed_dtypes(ops):
    V, e = 50257, Errors("kl views / unequal strides / mixed dtypes")
    big_t = (torch.randn(4, 33, V + 8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(21)) * 3.0).half()
    big_x = (big_t.float() + 0.1 * torch.randn_like(big_t, dtype=torch.float32)).half()
    t3, x3 = big_t[..., :V], big_x[..., :V]
    ref = kl_expr(x3.double(), t3.double())
    got = ops.eval_kl(x3, t3)
    e.add(got, ref, kl_expr(x3.float(), t3.float()))
    # the shifted views of compute_kl_div; a target with another row stride (element-wise path); other dtypes
    assert torch.equal(ops.eval_kl(x3[:, :-1], t3[:, :-1]), got[:, :-1])
    tc = t3.contiguous()
    assert tc.stride(1) != x3.stride(1)
    e.add(ops.eval_kl(x3, tc), ref, kl_expr(x3.float(), t3.float()))
    xb, tf = x3.to(torch.bfloat16), t3.float().contiguous()
    e.add(ops.eval_kl(xb, tf), kl_expr(xb.double(), tf.double()), kl_expr(xb.float(), tf))
    e.add(ops.eval_kl(tf, xb), kl_expr(tf.double(), xb.double()), kl_expr(tf, xb.float()))
    e.check()


def test_kl_special_values_follow_torch(ops):
    V = 4096
    for dt in DTYPES.values():
        t = make_logits(5, V, dt, seed=31).clone()
        x = (t.float() + 0.2 * torch.randn(5, V, device="cuda")).to(dt)
        x[1, 9] = float("nan")                                  # NaN in the logits -> NaN
        t[2, 1000] = float("nan")                               # NaN in the target -> NaN
        x[3, 7] = -float("inf")                                 # zero model probability under a positive target one -> +inf
        x[4, 2000:3000] = -float("inf"); t[4, 2000:3000] = -float("inf")  # noqa: E702  torch: 0 * (-inf - -inf) = NaN
        got, want = ops.eval_kl(x, t), kl_expr(x.float(), t.float())
        assert torch.isnan(got[[1, 2, 4]]).all() and torch.isnan(want[[1, 2, 4]]).all(), (got, want)
        assert got[3].item() == float("inf") == want[3].item()
        torch.testing.assert_close(got[0], want[0], rtol=0, atol=4e-6)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_kl_sparse_against_fp64(ops, dt):
    e = Errors(f"kl_sparse {dt}")
    for V, T, K, mode in ((128256, 2047, 32, "topk"), (128256, 3, 4096, "topk"), (32000, 2047, 1, "topk"),
                          (50257, 3, 32, "random"), (512, 2047, 4096, "random"), (512, 1, 32, "dup")):
        tl = make_logits(T, V, DTYPES[dt], seed=V + K)
        x = (tl.float() + 0.3 * make_logits(T, V, torch.float32, seed=K + T) / 3.0).to(DTYPES[dt])
        if mode == "topk":
            vals, ids = tl.topk(k=K, dim=-1)
        else:
            g = torch.Generator(device="cuda").manual_seed(K)
            ids = torch.randint(0, V, (T, K), device="cuda", generator=g)  # K = 4096 out of V = 512: every id repeats
            if mode == "dup":
                ids[:, 1::2] = ids[:, 0::2]
            vals = tl.gather(-1, ids)
        got = ops.eval_kl_sparse(x, vals, ids)
        xg = x.gather(-1, ids)
        e.add(got, kl_expr(xg.double(), vals.double()), kl_expr(xg.float(), vals.float()))
        if K > 1:
            assert bool((got > 0).all())
        del x, tl
    e.check()
    x = make_logits(4, 512, DTYPES[dt], seed=1)
    ids = torch.tensor([[0, 1], [2, 512], [-1, 3], [4, 5]], device="cuda")
    got = ops.eval_kl_sparse(x, torch.zeros(4, 2, device="cuda"), ids)  # an id outside [0, V) is not read: NaN row
    assert torch.isnan(got[[1, 2]]).all() and torch.isfinite(got[[0, 3]]).all()


# ------------------------------------------------------------------------------------------------ metrics on G17
class StubModel:
    def __init__(self, ids, logits):
        self.ids, self.table = ids, logits
        self.p = torch.nn.Parameter(torch.zeros(1, dtype=logits.dtype, device=logits.device))

    def parameters(self):
        return iter([self.p])

    def __call__(self, inputs):
        rows = [int((self.ids == r).all(dim=1).nonzero()[0, 0]) for r in inputs]
        return type("Out", (), {"logits": self.table[rows].clone()})()


@pytest.mark.parametrize("batch_size", [1, 2, 3])
def test_metrics_on_the_kernels_match_the_reference_floats(ops, batch_size):
    """The uploaded G17 logits through metrics.py on the real kernels.  The same rule: against the fp64 expression, the
    result may be off by at most 4 x what the reference's own fp32 run (the golden float) is off by."""
    from gptq_gguf_toolkit_amd import metrics
    g = load_golden("G17_eval")
    ids, tq, tt = (torch.from_numpy(g[k]).cuda() for k in ("ids", "quant_logits", "target_logits"))
    tv, ti = torch.from_numpy(g["topk_values"]).cuda(), torch.from_numpy(g["topk_indices"]).cuda()
    model, data = StubModel(ids, tq), [r[None] for r in ids]
    labels = ids[:, 1:].reshape(-1)
    rows64 = nll64(tq[:, :-1].reshape(-1, 512), labels)
    e = Errors(f"G17 rows, batch {batch_size}")
    e.add(metrics.nll_rows(model, data, batch_size), rows64, nll32(tq[:, :-1].reshape(-1, 512), labels))
    e.add(ops.eval_kl(tq[:, :-1], tt[:, :-1]), kl_expr(tq[:, :-1].double(), tt[:, :-1].double()), kl_expr(tq[:, :-1], tt[:, :-1]))
    e.check()
    exact = {"ppl": math.exp(float(rows64.mean())), "kl": float(kl_expr(tq[:, :-1].double(), tt[:, :-1].double()).mean()),
             "sparse_kl": float(kl_expr(tq[:, :-1].gather(-1, ti[:, :-1]).double(), tv[:, :-1].double()).mean())}
    got = {"ppl": metrics.compute_perplexity(model, data, batch_size),
           "kl": metrics.compute_kl_div(model, data, [t[None] for t in tt], batch_size),
           "sparse_kl": metrics.compute_sparse_kl_div(model, data, [(v[None], i[None]) for v, i in zip(tv, ti)])}
    for k in exact:
        ours, ref = abs(got[k] - exact[k]), abs(float(g[k]) - exact[k])
        print(f"[error_rule] G17 {k}: ours {got[k]!r} golden {float(g[k])!r} fp64 {exact[k]!r}: {ours:.3e} vs {ref:.3e}")
        assert ours <= 4 * ref, k
        assert abs(got[k] / float(g[k]) - 1) <= 1e-6, k


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def gguf_model(tmp_path_factory):
    """The recipe of tests/test_gpu_decode.py: a 2-layer random Llama (hidden 256, vocab 512), mixed K-quant types over the
    projections, embed and lm_head quantized: Quantizer.quantize -> convert -> .gguf.  Plus the evaluation ids.  One
    difference: the model that is quantized is LOADED from its saved directory, as ppleval and quant.py load it (a model
    built in fp32 and cast to fp16 carries a rotary table rounded to fp16, a loaded one does not: same weights, other logits)."""
    from pathlib import Path
    from make_golden_shim import MIXED, tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import convert
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    from gptq_gguf_toolkit_amd.quantizer import Quantizer
    tmp = tmp_path_factory.mktemp("eval")
    hf, sd = tmp / "hf", tmp / "q"
    tiny_llama(dtype=torch.float16).save_pretrained(str(hf), safe_serialization=True)
    model = load_hf(str(hf))
    data = [([], {"input_ids": ids}) for ids in tiny_calib()]
    Quantizer(model, data_loader=data, quantizable_modules=r".*layers.*((q|k|v|o|gate|up|down)_proj)$",
              quantizer_kwargs=dict(rel_damp=0.01, block_size=128, act_order=False, quant_scale="absmax", static_groups=False,
                                    rmin=-1.0, rdelta=0.1, nstep=20, verbose=False),
              pre_block_modules=["model.embed_tokens"], block_modules="model.layers", post_block_modules=["lm_head"],
              quant_non_block_modules=True, device="cuda:0", save_dir=str(sd)).quantize({k: T[v] for k, v in MIXED.items()})
    torch.cuda.synchronize()
    out = convert(Path(hf), Path(sd), tmp / "m.gguf", "f16", vocab=False)
    ids = tiny_calib(n=3, L=64, seed=29)
    torch.save(ids, str(tmp / "ids.pt"))
    return {"model": model, "gguf": str(out), "hf": str(hf), "tmp": tmp, "ids": ids, "ids_pt": str(tmp / "ids.pt")}


def load_hf(path):
    from transformers import AutoModelForCausalLM
    return AutoModelForCausalLM.from_pretrained(path, dtype=torch.float16, attn_implementation="eager").cuda().eval()


def run_ppleval(m, name, *extra, base=None):
    from gptq_gguf_toolkit_amd import ppleval
    out = m["tmp"] / f"{name}.json"
    argv = ["--model_name_or_path", base or m["hf"], "--eval_datasets", m["ids_pt"], "--sequence_length", "64", "--dtype", "float16",
            "--attn_implementation", "eager", "--output_file", str(out), *extra]
    with redirect_stdout(io.StringIO()):
        ppleval.main(argv)
    res = json.loads(out.read_text())
    args = ppleval.parse_args(argv)
    scored = ppleval.apply_weights(ppleval.load_hf_model(args, torch.device("cuda")), args)
    return res, scored


def test_ppleval_end_to_end(ops, gguf_model):
    from make_golden_shim import tiny_llama
    from gptq_gguf_toolkit_amd import gguf_splitter, metrics
    m = gguf_model
    live, ids, name = m["model"], m["ids"], m["ids_pt"]
    with torch.no_grad():
        logits = torch.cat([live(i.cuda()).logits for i in ids])  # [3, 64, 512] fp16
    labels = torch.cat(ids).cuda()[:, 1:].reshape(-1)
    rows64 = nll64(logits[:, :-1].reshape(-1, 512), labels)

    # --gguf, with the KL against the unmodified HF model
    res, scored = run_ppleval(m, "a", "--gguf", m["gguf"], "--kl_against", "model", "--eval_batch_size", "2")
    assert set(res) == {"model_name_or_path", "evaluation_config", "compression_config", "perplexity_results", "kl_results"}
    assert res["evaluation_config"]["dtype"] == "torch.float16" and res["compression_config"]["gguf"] == m["gguf"]
    rows_a = metrics.nll_rows(scored, ids)
    e = Errors("ppleval --gguf rows")
    e.add(rows_a, rows64, nll32(logits[:, :-1].reshape(-1, 512), labels))
    ppl_a = res["perplexity_results"][name]
    assert abs(ppl_a / math.exp(float(rows_a.double().mean())) - 1) < 1e-12  # the JSON is the mean of exactly these rows
    print(f"\nppleval --gguf: {ppl_a!r}; exp(F.cross_entropy(logits.double())) = {math.exp(float(rows64.mean()))!r}")
    orig = load_hf(m["hf"])
    with torch.no_grad():
        t_logits = torch.cat([orig(i.cuda()).logits for i in ids])
    kl_rows = ops.eval_kl(logits[:, :-1], t_logits[:, :-1])
    kl64 = kl_expr(logits[:, :-1].double(), t_logits[:, :-1].double())
    e.add(kl_rows, kl64, kl_expr(logits[:, :-1].float(), t_logits[:, :-1].float()))
    e.check()
    kl_a = res["kl_results"][name]
    assert kl_a > 0 and abs(kl_a / float(kl_rows.double().mean()) - 1) < 1e-12
    print(f"ppleval --kl_against model: {kl_a!r}; fp64 expression {float(kl64.mean())!r}")

    # --kl_against the file itself: exactly 0
    res0, _ = run_ppleval(m, "z", "--gguf", m["gguf"], "--kl_against", f"gguf:{m['gguf']}")
    assert res0["kl_results"][name] == 0.0 and res0["perplexity_results"][name] == ppl_a

    # the --hf-layers database, default level: every projection from "0.pth" over a base that holds the file's embed / lm_head
    db0, db1 = m["tmp"] / "db0", m["tmp"] / "db1"
    gguf_splitter.main([m["gguf"], str(db0), "--hf-layers", "--dtype", "float16", "--bitwidth", "0"])
    gguf_splitter.main([m["gguf"], str(db1), "--hf-layers", "--dtype", "float16"])
    assert (db0 / "model.layers.0.self_attn.q_proj" / "0.pth").is_file()
    assert (db1 / "model.layers.0.self_attn.q_proj" / "3-Q3_K.pth").is_file()
    qsd = live.state_dict()
    base0 = tiny_llama(dtype=torch.float16)
    sd0 = base0.state_dict()
    for k in ("model.embed_tokens.weight", "lm_head.weight"):
        assert not torch.equal(sd0[k], qsd[k].cpu())
        sd0[k] = qsd[k].cpu()
    base0.load_state_dict(sd0)
    base0.save_pretrained(str(m["tmp"] / "base0"), safe_serialization=True)
    res_b, scored_b = run_ppleval(m, "b", "--quant_weights_path", str(db0), base=str(m["tmp"] / "base0"))
    # ... and a two-line config in both level spellings over a base that lacks exactly those two layers
    two = ("model.layers.0.self_attn.q_proj", "model.layers.1.mlp.up_proj")
    base1 = tiny_llama(dtype=torch.float16)
    sd1 = {k: v.cpu().clone() for k, v in qsd.items()}
    for n in two:
        sd1[n + ".weight"] = tiny_llama(dtype=torch.float16).state_dict()[n + ".weight"]
    base1.load_state_dict(sd1)
    base1.save_pretrained(str(m["tmp"] / "base1"), safe_serialization=True)
    cfg = m["tmp"] / "levels.txt"
    cfg.write_text(f"{two[0]}: 3\n{two[1]}: 4-Q4_K\n")
    res_c, scored_c = run_ppleval(m, "c", "--quant_weights_path", str(db1), "--quant_config_path", str(cfg),
                                  base=str(m["tmp"] / "base1"))
    res_d, _ = run_ppleval(m, "d", base=str(m["tmp"] / "base1"))  # without the config the two layers are the original ones
    assert res_d["perplexity_results"][name] != ppl_a
    # the decoded weights are bit-identical, so the per-row values are: equality, not closeness
    for r, s in ((res_b, scored_b), (res_c, scored_c)):
        assert torch.equal(metrics.nll_rows(s, ids), rows_a)
        assert r["perplexity_results"][name] == ppl_a and "kl_results" not in r


def test_quant_cli_eval_perplexity_on_eval_data(ops, gguf_model):
    """quant.py --eval_perplexity --eval_data on the fixture's model and settings prints the perplexity of the quantized
    model: the same number as the fixture's own (bit-identically) quantized model gives."""
    from make_golden_shim import MIXED
    from gptq_gguf_toolkit_amd import metrics, quant
    m = gguf_model
    tmp = m["tmp"]
    from make_golden_shim import tiny_calib
    torch.save(tiny_calib(), str(tmp / "calib.pt"))
    (tmp / "bits.json").write_text(json.dumps(MIXED))
    buf = io.StringIO()
    with redirect_stdout(buf):
        quant.main(["--model_name_or_path", m["hf"], "--quantizable_modules", r".*layers.*((q|k|v|o|gate|up|down)_proj)$",
                    "--pre_block_modules", "model.embed_tokens", "--block_modules", "model.layers",
                    "--post_block_modules", "lm_head", "--quant_non_block_modules", "--calibration_data", str(tmp / "calib.pt"),
                    "--calibration_tokens", str(8 * 64), "--calibration_sequence_length", "64", "--quant_scale", "absmax",
                    "--rel_damp", "0.01", "--block_size", "128", "--bit_width_configuration", str(tmp / "bits.json"),
                    "--dtype", "float16", "--seed", "0", "--attn_implementation", "eager", "--save_dir", str(tmp / "cli_q"),
                    "--eval_perplexity", "--eval_data", m["ids_pt"], "--eval_sequence_length", "64"])
    out = buf.getvalue()
    assert "Quantization took" in out
    hit = re.search(r"^Perplexity on ids\.pt: (\d+\.\d{3})$", out, re.M)
    assert hit, out
    want = metrics.compute_perplexity(m["model"], m["ids"])
    print(f"\nquant.py printed {hit.group(1)}; the live quantized model scores {want!r}")
    assert hit.group(1) == f"{want:.3f}"
