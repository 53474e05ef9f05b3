"""-m gpu: fused-expert MoE models through the Quantizer on the GPU.  gq_fwd_moe_combine against the loop restatement of
its contract (tests/moe_combine_spec.py), byte for byte, and against transformers' own launch sequence on the device;
CalibExperts' "routed" forward against transformers' MixtralExperts.forward, with the first-input verification on both
outcomes; the driver on a tiny transformers-5.x Mixtral against the oracle-backed run of the same model; quantize -> pack ->
load back."""
import os
import sys
from pathlib import Path

import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests"))

from moe_combine_spec import bits, combine_hf, combine_spec, route, transposed_pairs  # noqa: E402
import test_moe_quantize_cpu as host  # noqa: E402

E = 5
# Share of differing integers of the expert Linears between the GPU run and the oracle-backed CPU run of the same model and
# calibration ids: the largest rate measured on an MI355X (layers.1 experts.0.w2, Q4_K; the mean over the 30
# expert Linears is 0.024 %), and the cap: twice the measured value, rounded up to one significant digit.
EXPERT_RATE_MEASURED = 0.002251
EXPERT_RATE_CAP = 0.005


# ------------------------------------------------------------------------------------------------ the kernel
def run_kernel(y, idx, w):
    from gptq_gguf_toolkit_amd import ops
    pairs = idx.t().contiguous().view(-1).to(torch.int32).cuda()
    rt = ops.moe_route(pairs, E)
    start, order = route(transposed_pairs(idx), E)
    assert rt[0].tolist() == start and rt[1].tolist() == order
    return ops.fwd_moe_combine(y.cuda(), pairs, rt, w.cuda(), E)


@pytest.mark.parametrize("w_kind", ["w-fp32", "w-act"])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_combine_is_the_contract_and_transformers_sequence(dt, w_kind):
    """Per (T, K, H): a plain case; an edge case (expert 4 unused, one pair with id = E, one token with every pair masked, a
    first product that is -0); a case where a token names one expert twice (against the contract only: index_add_ leaves the
    order of two rows of one call open).  K = 8 of 5 experts repeats experts in every token."""
    w_dt = torch.float32 if w_kind == "w-fp32" else dt
    for T in (1, 7, 96):
        for Kc in (1, 2, 8):
            for Hc in (8, 264, 256):
                cases = [("plain", host.combine_case(T, Kc, E, Hc, dt, w_dt, seed=T + Kc)),
                         ("edge", host.combine_case(T, Kc, E, Hc, dt, w_dt, seed=1, unused=4, masked=[(3, Kc - 1)] if T > 3 else (),
                                                    all_masked=5 if T > 5 else None, neg_zero=True)),
                         ("twice", host.combine_case(T, Kc, E, Hc, dt, w_dt, seed=2, twice=T - 1))]
                for name, (y, idx, w) in cases:
                    got = run_kernel(y, idx, w)
                    what = (name, T, Kc, Hc)
                    assert got.dtype == dt and got.shape == (T, Hc)
                    assert torch.equal(bits(got.cpu()), bits(combine_spec(y, idx, w, E))), what
                    if name == "edge":
                        assert int(bits(got.cpu())[0, 0]) == 0, what  # +0, not the -0 of the product
                        assert T <= 5 or bool((bits(got.cpu())[5] == 0).all()), what
                    if Kc <= 2 and name != "twice":  # no token names an expert twice: transformers' result, bit for bit
                        assert torch.equal(bits(got), bits(combine_hf(y.cuda(), idx.cuda(), w.cuda(), E))), what


# ------------------------------------------------------------------------------------------------ "routed" against the module
def hf_block(dt):
    import moe_gguf
    from transformers.models.mixtral.modeling_mixtral import MixtralSparseMoeBlock
    torch.manual_seed(0)
    holder = torch.nn.Module()
    holder.mlp = MixtralSparseMoeBlock(moe_gguf.config()).eval()
    with torch.no_grad():
        for p in holder.mlp.experts.parameters():
            p.copy_(torch.randn(p.shape) * 0.05)
    return holder.to(dt).cuda()


def routing(T, seed):
    import moe_gguf
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, moe_gguf.H, generator=g)
    idx = torch.stack([torch.randperm(moe_gguf.E, generator=g)[:moe_gguf.K] for _ in range(T)])
    w = torch.softmax(torch.randn(T, moe_gguf.K, generator=g), -1)  # fp32, as the router leaves it
    return x, idx.cuda(), w.cuda()


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_routed_forward_is_transformers_forward(dt, monkeypatch):
    from gptq_gguf_toolkit_amd import moe_calibration as mc
    from gptq_gguf_toolkit_amd import ops
    holder = hf_block(dt)
    orig = holder.mlp.experts
    eager = type(orig).forward.__wrapped__  # MixtralExperts.forward's own loop, whatever implementation the config names
    installed = mc.install(holder, "mlp.", r"experts\.\d+\.w[123]$", "routed")
    stand_in = holder.mlp.experts
    mc.reset_verdicts()
    calls = []
    real = ops.fwd_moe_combine
    monkeypatch.setattr(ops, "fwd_moe_combine", lambda *a: calls.append(1) or real(*a))
    fed = []
    for n, m in holder.named_modules():
        if isinstance(m, torch.nn.Linear):
            m.register_forward_pre_hook(lambda mod, inp, n=n: fed.append((n, inp[0])))
    with torch.no_grad():
        for T in (1, 96):
            for seed in (T, T + 1, T + 2):  # the first input of the class verifies, the later ones take the routed forward alone
                x, idx, w = routing(T, seed)
                x = x.to(dt).cuda()
                del fed[:]
                n_calls = len(calls)
                got = stand_in(x, idx, w)
                assert torch.equal(got, eager(orig, x, idx, w)), (T, seed)
                assert len(calls) == n_calls + 1  # verification and trusted use both run the kernel once
                hit = sorted(set(idx.flatten().tolist()))
                assert [n for n, _ in fed] == [f"mlp.experts.{e}.{r}" for e in hit for r in ("w1", "w3", "w2")]  # once each
                for e in hit:
                    _, token_idx = torch.where((idx == e).T)
                    x1, x3 = fed[3 * hit.index(e)][1], fed[3 * hit.index(e) + 1][1]
                    assert torch.equal(x1, x[token_idx]) and x1.data_ptr() == x3.data_ptr()
            assert mc._routed_verdict[(T, 2, 4, 256, 512, dt)] is True
        # the failing outcome: a combine that returns one wrong bit leaves the class on "loop"
        mc.reset_verdicts()

        def wrong(*a):
            out = real(*a)
            out.view(torch.int16)[0, 0] ^= 1
            return out

        monkeypatch.setattr(ops, "fwd_moe_combine", wrong)
        for seed in (7, 8):
            x, idx, w = routing(96, seed)
            x = x.to(dt).cuda()
            assert torch.equal(stand_in(x, idx, w), eager(orig, x, idx, w))
        assert mc._routed_verdict[(96, 2, 4, 256, 512, dt)] is False
        monkeypatch.setattr(ops, "fwd_moe_combine", real)
    mc.restore(installed)
    mc.reset_verdicts()
    assert holder.mlp.experts is orig


# ------------------------------------------------------------------------------------------------ the driver
@pytest.fixture(scope="module")
def both_runs(tmp_path_factory):
    """The same tiny Mixtral (fp32) and calibration ids through the Quantizer twice: on the CPU with tests/fake_ops.py (the
    oracle) as the backend, and on the GPU."""
    import fake_ops
    tmp = tmp_path_factory.mktemp("moe_gpu")
    cpu_dir, gpu_dir = tmp / "cpu", tmp / "gpu"
    os.makedirs(cpu_dir), os.makedirs(gpu_dir)
    with pytest.MonkeyPatch.context() as mp:
        fake_ops.install(mp)
        host.make_quantizer(host.tiny_mixtral(), cpu_dir).quantize(host.qconfig())
    model = host.tiny_mixtral().cuda()
    experts = [layer.mlp.experts for layer in model.model.layers]
    host.make_quantizer(model, gpu_dir, device="cuda:0").quantize(host.qconfig())
    torch.cuda.synchronize()
    assert all(layer.mlp.experts is m for layer, m in zip(model.model.layers, experts))
    return str(cpu_dir), str(gpu_dir), model


def test_driver_on_gpu_against_the_oracle_backed_run(both_runs):
    cpu_dir, gpu_dir, model = both_runs
    names = host.tree_names()
    assert sorted(os.listdir(gpu_dir)) == names == sorted(os.listdir(cpu_dir))
    rates = {}
    for n in names:
        a, five_a = host.load_tree(cpu_dir, n)
        b, five_b = host.load_tree(gpu_dir, n)
        assert a["q_type"] == b["q_type"]
        assert all(x.shape == y.shape and x.dtype == y.dtype and not y.is_cuda for x, y in zip(five_a, five_b)), n
        exact = n in ("model.embed_tokens", "lm_head") or f".experts.{host.E5 - 1}." in n  # RTN / H = I: no Hessian behind them
        if exact:
            assert all(torch.equal(x, y) for x, y in zip(five_a, five_b)), n
        rates[n] = float((five_a[0] != five_b[0]).float().mean())
    print("\n[GPU run vs oracle-backed run] share of differing ints per module:")
    for n, r in rates.items():
        print(f"    {n:50s} {r:.4%}")
    attn = {n: r for n, r in rates.items() if "self_attn" in n}
    experts = {n: r for n, r in rates.items() if ".experts." in n}
    print(f"    attention max {max(attn.values()):.4%}  experts max {max(experts.values()):.4%}  "
          f"experts mean {sum(experts.values()) / len(experts):.4%}")
    # the caps of tests/test_driver_gpu.py for Linears fed by every token
    assert max(attn.values()) < 0.04 and max(r for n, r in attn.items() if ".layers.0." in n) < 0.002, attn
    # expert Linears see K / E of the tokens, some fewer rows than columns
    assert max(experts.values()) < EXPERT_RATE_CAP, experts
    with torch.no_grad():
        logits = model(host.calib()[0].cuda()).logits
    assert bool(torch.isfinite(logits).all())


def test_quantize_pack_load_round_trip(tmp_path):
    """fp16 on the GPU (the routed forward, verified on its first input): Q4_K everywhere -> pack_gptq_into_gguf ->
    gguf_loader.load_into_model: the loaded fused parameters are the quantizer's written-back weights, as 16-bit patterns."""
    from transformers import AutoModelForCausalLM
    from gptq_gguf_toolkit_amd import gguf_loader
    from gptq_gguf_toolkit_amd import moe_calibration as mc
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import convert
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    hf, save = tmp_path / "hf", tmp_path / "tree"
    host.tiny_mixtral().half().save_pretrained(str(hf), safe_serialization=True)
    os.makedirs(save)

    def load():
        return AutoModelForCausalLM.from_pretrained(str(hf), dtype=torch.float16, attn_implementation="eager").cuda().eval()

    model = load()
    host.make_quantizer(model, save, device="cuda:0").quantize({k: T.Q4_K for k in host.QCFG})
    torch.cuda.synchronize()
    assert mc.ROUTED_LEVELS and mc._routed_verdict and all(mc._routed_verdict.values()), mc._routed_verdict
    assert sorted(os.listdir(save)) == host.tree_names()
    out = convert(Path(hf), Path(save), tmp_path / "m.gguf", "f16", vocab=False)
    loaded = gguf_loader.load_into_model(load(), str(out))
    want, got = dict(model.named_parameters()), dict(loaded.named_parameters())
    checked = 0
    for n in want:
        if n.endswith(("experts.gate_up_proj", "experts.down_proj")):
            assert torch.equal(bits(want[n].detach()), bits(got[n].detach())), n
            checked += 1
    assert checked == host.LAYERS * 2
