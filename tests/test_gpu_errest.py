"""-m gpu: gq_quad_form (K17) and the layer error estimator on the GPU.

Accuracy rule (tests/test_gpu_eval.py's): the anchor is the torch expression in fp64 on the same device tensors; over a
whole case set the kernel's largest relative error must stay within 4 x the largest relative error of torch's own fp32
expression ((D @ H) * D).sum(), measured in the same test with TF32 off.  The structure checks are exact in fp32 by
construction and are compared bit for bit (or to a few fp32 ulp where one rounding per product remains)."""
import ctypes
import os
import sys

import pytest

from conftest import ROOT, load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

CASES = ((1, 128), (130, 256), (64, 768), (257, 1280))  # one diagonal block + a one-row tile; one off-diagonal block + a
# ragged second row tile; odd block count, triangular costs; more tiles than one round of workgroups takes at once
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
SIGMAS = (1e-1, 1e-2, 1e-3)
ULP = 2.0 ** -23


def _ops():
    from gptq_gguf_toolkit_amd import ops
    return ops


def _fix(H):
    H = H.clone()
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    return H


def _d32(A, B):
    return A.float() - B.float() if B is not None else A.float()


def quad64(A, H, B=None):
    D = _d32(A, B).double()
    return float(((D @ _fix(H).double()) * D).sum())


def quad32(A, H, B=None):
    assert torch.backends.cuda.matmul.allow_tf32 is False and torch.get_float32_matmul_precision() == "highest"
    D = _d32(A, B)
    return float(((D @ _fix(H)) * D).sum())


def _bytes(t):
    return t.view(torch.int64).item()


_made = {}


def inputs(R, C):
    """(A fp32, noise fp32, H) of a case, made once: H = (2/T) X^T X from the package's own SYRK, T = 2 C."""
    if (R, C) not in _made:
        g = torch.Generator(device="cuda").manual_seed(1000 * R + C)
        X = torch.randn(2 * C, C, generator=g, device="cuda").half()
        H = _ops().h_accumulate(torch.zeros(C, C, device="cuda"), X, 0.0, 2.0 / (2 * C))
        assert torch.equal(H, H.T)
        A = torch.randn(R, C, generator=g, device="cuda") * 0.05
        _made[(R, C)] = (A, torch.randn(R, C, generator=g, device="cuda"), H)
    return _made[(R, C)]


def test_accuracy_against_fp64_over_the_case_set():
    ops = _ops()
    worst_k, worst_t, n = 0.0, 0.0, 0
    for R, C in CASES:
        A32, noise, H = inputs(R, C)
        rms = float(A32.pow(2).mean().sqrt())
        for da in DTYPES:
            A = A32.to(da)
            todo = [None] + [(A32 + s * rms * noise).to(db) for db in DTYPES for s in SIGMAS]
            for B in todo:
                want = quad64(A, H, B)
                ek = abs(_ops().quad_form(A, H, B).item() - want) / abs(want)
                et = abs(quad32(A, H, B) - want) / abs(want)
                worst_k, worst_t, n = max(worst_k, ek), max(worst_t, et), n + 1
    print(f"quad_form: {n} calls, largest relative error kernel {worst_k:.3e}, torch fp32 {worst_t:.3e}")
    assert worst_t > 0 and worst_k <= 4 * worst_t
    out = ops.quad_form(A, H)
    assert out.dtype == torch.float64 and out.dim() == 0 and out.is_cuda


@pytest.mark.parametrize("R,C", CASES)
def test_identity_gives_the_squared_norm(R, C):
    A32, noise, _ = inputs(R, C)
    H = torch.eye(C, device="cuda")
    for A, B in ((A32, None), (A32.half(), (A32 + 0.01 * noise).bfloat16())):
        want = float(_d32(A, B).double().pow(2).sum())
        got = _ops().quad_form(A, H, B).item()
        assert abs(got - want) <= 2 * ULP * want  # d * 1 is exact; one fp32 rounding per product d * d, sums in fp64


@pytest.mark.parametrize("R,C", CASES[1:])
def test_diagonal_and_off_diagonal_blocks_add_up_exactly(R, C):
    """Small integers: every product and sum is exact in fp32, so the three results are exact and
    full == diagonal blocks + off-diagonal blocks bit for bit (a wrong weight 2 or a block counted twice shows)."""
    g = torch.Generator(device="cuda").manual_seed(7 * R + C)
    S = torch.randint(-3, 4, (C, C), generator=g, device="cuda").float()
    H = torch.triu(S, 1) + torch.triu(S, 1).T + torch.diag(torch.randint(1, 4, (C,), generator=g, device="cuda").float())
    blk = torch.arange(C, device="cuda") // 128
    on = (blk[:, None] == blk[None, :]).float()
    A = torch.randint(-4, 5, (R, C), generator=g, device="cuda").float()
    B = torch.randint(-2, 3, (R, C), generator=g, device="cuda").half()
    ops = _ops()
    full, diag, off = ops.quad_form(A, H, B), ops.quad_form(A, H * on, B), ops.quad_form(A, H * (1 - on), B)
    assert full.item() == quad64(A, H, B) and diag.item() == quad64(A, H * on, B)
    # the off-diagonal part has a zero diagonal, which reads as 1: that identity term (exact too) comes out again
    norm2 = ops.quad_form(A, torch.eye(C, device="cuda"), B)
    assert off.item() == quad64(A, H * (1 - on), B) and norm2.item() == float(_d32(A, B).double().pow(2).sum())
    assert _bytes(diag + (off - norm2)) == _bytes(full)


def test_dead_channel_reads_as_one_and_H_is_not_written():
    R, C = 130, 256
    A32, noise, H0 = inputs(R, C)
    H = H0.clone()
    for i in (70, 128 + 5):  # inside a diagonal block, one in each
        H[i, :] = 0
        H[:, i] = 0
    keep = H.clone()
    H1 = H.clone()
    H1[70, 70] = 1
    H1[133, 133] = 1
    ops = _ops()
    for A, B in ((A32, None), (A32.half(), (A32 + 0.01 * noise).half())):
        assert float(_d32(A, B)[:, 70].abs().min()) > 0
        got, want = ops.quad_form(A, H, B), ops.quad_form(A, H1, B)
        assert _bytes(got) == _bytes(want)
        assert abs(got.item() - quad64(A, H1, B)) <= 1e-5 * quad64(A, H1, B)
        assert ops.quad_form(A, H0, B).item() != got.item()
    assert torch.equal(H, keep)


def test_same_bytes_twice_and_whatever_the_workspace_held():
    ops = _ops()
    from gptq_gguf_toolkit_amd import _cabi
    for R, C in CASES:
        A32, noise, H = inputs(R, C)
        A, B = A32.half(), (A32 + 0.01 * noise).half()
        first = _bytes(ops.quad_form(A, H, B))
        assert _bytes(ops.quad_form(A, H, B)) == first
        need = int(_cabi.lib().gq_quad_form_workspace_bytes(R, C))
        for fill in (0xFF, 0x00):
            ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
            assert _bytes(ops.quad_form(A, H, B, ws=ws)) == first


def test_row_views_are_read_in_place():
    R, C = 130, 256
    A32, noise, H = inputs(R, C)
    ops = _ops()
    for dt in DTYPES:
        wide = torch.zeros(R, C + 64, dtype=dt, device="cuda")
        wide[:, :C] = A32.to(dt)
        wide[:, C:] = 7.0  # never read
        view = wide[:, :C]
        assert not view.is_contiguous() and ops._qf_rows(view).data_ptr() == view.data_ptr()  # handed on, lda = C + 64
        Bw = torch.zeros(R, C + 128, dtype=torch.float16, device="cuda")
        Bw[:, :C] = (A32 + 0.01 * noise).half()
        assert _bytes(ops.quad_form(view, H, Bw[:, :C])) == _bytes(ops.quad_form(view.contiguous(), H, Bw[:, :C].contiguous()))
    # rows that are not 16-byte aligned are copied by the op (and refused by the library, below)
    odd = torch.zeros(R, C + 8, dtype=torch.float16, device="cuda")
    odd[:, 1:C + 1] = A32.half()
    assert ops._qf_rows(odd[:, 1:C + 1]).data_ptr() != odd[:, 1:C + 1].data_ptr()
    assert _bytes(ops.quad_form(odd[:, 1:C + 1], H)) == _bytes(ops.quad_form(A32.half(), H))


def test_refusals():
    from gptq_gguf_toolkit_amd import _cabi
    ops = _ops()
    A32, _, H = inputs(130, 256)
    with pytest.raises(_cabi.GQError, match="C=192"):
        ops.quad_form(torch.zeros(4, 192, device="cuda"), torch.zeros(192, 192, device="cuda"))
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.quad_form(A32.cpu(), H)
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.quad_form(A32, H, A32.cpu())
    with pytest.raises(_cabi.GQError):
        ops.quad_form(A32, H, A32[:64])
    # a misaligned view, handed to the library as it is: refused before anything is launched
    A = A32.half()
    out, ws = torch.zeros((), dtype=torch.float64, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")
    vp = ctypes.c_void_p
    with pytest.raises(_cabi.GQError, match="rows of A"):
        _cabi.check(_cabi.lib().gq_quad_form(vp(A.data_ptr() + 2), 1, 256, vp(0), 0, 0, vp(H.data_ptr()), 129, 256,
                                             vp(out.data_ptr()), vp(ws.data_ptr()), 64, vp(0)), "gq_quad_form")
    assert out.item() == 0.0


# ------------------------------------------------------------------------------------------------ fixture and driver
def _fp64_H(xs):
    C = xs[0].shape[-1]
    H, n = torch.zeros(C, C, dtype=torch.float64, device=xs[0].device), 0
    for x in xs:
        x2, b = x.reshape(-1, C).double(), x.shape[0]
        H = H * (n / (n + b)) + (2.0 / (n + b)) * (x2.T @ x2)
        n += b
    return H


def _fp32_H(xs):
    """The reference's update(), error_estimator.py:63-69."""
    C = xs[0].shape[-1]
    H, n = torch.zeros(C, C, dtype=torch.float32, device=xs[0].device), 0
    for x in xs:
        x2, b = x.reshape(-1, C).float(), x.shape[0]
        H.addmm_(x2.T, x2, beta=n / (n + b), alpha=2.0 / (n + b))
        n += b
    return H


def test_fixture_through_the_layer_estimator():
    from gptq_gguf_toolkit_amd.error_estimator import LayerErrorEstimator
    g = load_golden("G18_errest")
    xs = [torch.from_numpy(x).float().cuda() for x in g["inputs"]]
    layer = torch.nn.Linear(256, 48).cuda()
    layer.weight.data = torch.from_numpy(g["W"]).cuda()
    W = layer.weight.detach()
    h = LayerErrorEstimator(layer)
    for x in xs:
        h.update(x)
    h.pre_step()
    assert float(h.H[int(g["dead"]), int(g["dead"])]) == 0.0
    H64 = _fp64_H(xs)
    bound = 4 * float(g["rel_dist"].max())  # the reference's own fp32 distance from the same fp64 expression, x 4
    worst = 0.0
    for w_c, ref in zip(g["W_c"], g["errors"]):
        w_c = torch.from_numpy(w_c).cuda()
        got = h.estimate(w_c)
        assert got.is_cuda and got.dtype == torch.float64
        D = (W - w_c).double()
        Hf = _fix(H64)
        want = float(((D @ Hf) * D).sum() / ((W.double() @ Hf) * W.double()).sum())
        rel = abs(got.item() - want) / want
        worst = max(worst, rel)
        print(f"G18: kernel {got.item()!r} fp64 {want!r} reference {float(ref)!r} rel {rel:.3e} (bound {bound:.3e})")
    assert worst <= bound


def test_driver_on_the_tiny_llama(tmp_path):
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd.error_estimator import ErrorEstimator
    ops = _ops()
    model = tiny_llama().cuda()
    data = [([], {"input_ids": ids}) for ids in tiny_calib()]
    names = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and ".layers." in n]
    levels = (("2-Q2_K.pth", 10), ("4-Q4_K.pth", 12))  # RTN levels made here, stored in fp16
    for n in names:
        W = model.get_submodule(n).weight.detach().contiguous()
        os.makedirs(tmp_path / n)
        for f, qt in levels:
            torch.save(ops.dequantize(qt, *ops.rtn_quantize(W, qt)).half().cpu(), str(tmp_path / n / f))
    acts, hooks = {}, []
    for n in names:
        hooks.append(model.get_submodule(n).register_forward_hook(
            lambda m, inp, out, n=n: acts.setdefault(n, []).append(inp[0].detach().clone())))
    with torch.no_grad():
        for _, kw in data:
            model(input_ids=kw["input_ids"].cuda())
    for h in hooks:
        h.remove()

    est = ErrorEstimator(model, data, r".*layers.*((q|k|v|o|gate|up|down)_proj)$", ["model.embed_tokens"],
                         "model.layers", str(tmp_path), device="cuda:0")
    errors = est.estimate()[-1]
    assert sorted(errors) == sorted(names) and est.hessians_built == 8
    worst_k = worst_t = 0.0
    for n in names:
        assert est.levels[n] == [f for f, _ in levels]
        lo, hi = errors[n]
        assert 0 < hi < lo < 1 and lo == lo and hi == hi  # finite, and the 2-bit level hurts more than the 4-bit one
        W = model.get_submodule(n).weight.detach()
        H64, H32 = _fp64_H(acts[n]), _fp32_H(acts[n])
        for (f, _), got in zip(levels, errors[n]):
            w_c = torch.load(str(tmp_path / n / f)).cuda()
            want = quad64(W, H64, w_c) / quad64(W, H64)
            t32 = quad32(W, H32, w_c) / quad32(W, H32)
            worst_k, worst_t = max(worst_k, abs(got - want) / want), max(worst_t, abs(t32 - want) / want)
    print(f"driver: largest relative error kernel path {worst_k:.3e}, torch fp32 path {worst_t:.3e}")
    assert worst_t > 0 and worst_k <= 4 * worst_t
