"""-m gpu, round 4:
  * K3 (gptq.py:304-324, linalg_utils.py:8-12) on CORRELATED, ill-conditioned Hessians: the default image chain against
    the fp64 chain and against the all-fp32 chain (the reference's precision) on the same matrix -- row-wise error of U,
    the non-PD flag, and the end-to-end ints rate on a 128-row slice of down_proj 4096 x 14336 through the oracle;
  * the one shim of the bit-exact anchor (tests/golden/make_golden.py:73-90): torch.sqrt on the ROCm device is
    correctly rounded, which is what the "ieee" fixtures assume of the reference's GPU execution (quant_utils.py:204).
"""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)
from corr_hessian import CHAIN_MODES, correlated_x, env, fp64_chain, u_errors

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from gptq_gguf_toolkit_amd import ops as _ops
    return _ops


# ----------------------------------------------------------------- the shim: IEEE sqrt on the device
def test_torch_sqrt_on_the_device_is_correctly_rounded():
    """make_k_quants' `torch.sqrt(sum_x2 / G)` (quant_utils.py:204).  The CPU build of torch routes fp32 sqrt through MKL
    VML (1 ulp low on 0.6 % of inputs), so the golden fixtures were generated with an IEEE sqrt in its place, on the
    premise that the reference's GPU execution rounds correctly.  Pinned here on the box: 10^7 random positive fp32 bit
    patterns (denormals included) + edge values, against sqrt in fp64 rounded once to fp32 -- innocuous double
    rounding, 53 >= 2 * 24 + 2 -- computed on the host by numpy (sqrtsd)."""
    rng = np.random.default_rng(2024)
    bits = rng.integers(0, 0x7F800000, size=10_000_000, dtype=np.uint32)  # every finite non-negative fp32 pattern
    edge = np.array([0.0, -0.0, np.inf, 1.0, 2.0, 4.0, 1e-45, 1.1754942e-38, 1.17549435e-38, 3.4028235e38, 0.25,
                     16777216.0, 16777218.0, 2.0 ** -126, 2.0 ** -149, 1e-12, 4e-4, 0.02 ** 2], np.float32)
    # neighbours of perfect squares: where a 1-ulp-low sqrt shows first
    k = rng.integers(1, 4096, size=200_000).astype(np.float32)
    sq = (k * k)
    near = np.concatenate([sq, np.nextafter(sq, np.float32(0)), np.nextafter(sq, np.float32(np.inf))])
    # the magnitudes the path feeds it: mean squares of N(0, 0.02^2) weights
    w = (rng.standard_normal(2_000_000).astype(np.float32) * np.float32(0.02)) ** 2
    x = np.concatenate([bits.view(np.float32), edge, near, w])
    want = np.sqrt(x.astype(np.float64)).astype(np.float32)
    got = torch.sqrt(torch.from_numpy(x).cuda()).cpu().numpy()
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (int(bad.sum()), x[bad][:5], got[bad][:5], want[bad][:5])
    # the same in the model dtypes of the RTN path (quantizer.py:109,195: make_*quants in fp16 / bf16): ATen computes in
    # fp32 and rounds once to the tensor dtype
    for dt in (torch.float16, torch.bfloat16):
        xs = torch.from_numpy(x[:2_000_000]).cuda().to(dt)
        got = torch.sqrt(xs)
        want = torch.from_numpy(np.sqrt(xs.float().cpu().numpy().astype(np.float64)).astype(np.float32)).to(dt)
        assert torch.equal(got.cpu(), want), dt


# ----------------------------------------------------------------- K3 where it matters
def _h_of(ops, X, n_samples=8):
    C = X.shape[1]
    H = torch.zeros(C, C, device="cuda")
    ops.h_accumulate(H, X, 0.0, 2.0 / n_samples)
    return H


def _chain(ops, H, W, mode):
    with env(**CHAIN_MODES[mode]):
        Hc = H.clone()
        U, flag = ops.h_prepare(Hc, W.clone(), 0.01)
    return U, int(flag.item()), Hc


CORR_CASES = [  # (C, T, rank, eps, massive channels, mean shift): T < C and T >= C, rank C/16 and C/64, eps 0.3 and 0.03
    (4096, 2048, 256, 0.3, 6, 0.0),      # massive channels inflate the damping: cond(equilibrated, damped) ~ 1e1
    (4096, 2048, 64, 0.03, 0, 0.0),      # ~ 1.5e4
    (4096, 8192, 256, 0.03, 0, 3.0),     # un-centred activations: ~ 3e6
    (4096, 8192, 64, 0.3, 0, 3.0),       # ~ 2e6
    (14336, 7168, 896, 0.03, 6, 0.0),    # ~ 5e1
    (14336, 7168, 224, 0.3, 0, 3.0),     # ~ 1.1e7
    (14336, 28672, 896, 0.3, 0, 0.0),    # ~ 1.5e3
    (14336, 28672, 224, 0.03, 0, 3.0),   # ~ 1.4e7
]


@pytest.mark.parametrize("C,T,rank,eps,massive,mean", CORR_CASES)
def test_image_chain_on_correlated_hessians(ops, C, T, rank, eps, massive, mean):
    """X = Z_r A + eps Z (+ 6 channels x 1e3 | + a constant offset): the equilibrated, damped matrix the chain factorises
    has cond 1e1 ... 1.4e7 (profiles/r04_chol_corr_probe.txt lists cond and all three forms per case).
    (i) the default chain's error of U against the fp64 chain -- row-wise and in the max norm -- is at most 1.25 x that of the
    all-fp32 chain (options chol_fp32 + chol_3p_min = 0: image levels off = the reference's precision, linalg_utils.py:8-12) on the same matrix.
    Measured: 0.1 - 0.7 x everywhere -- the 16-bit MFMAs add 32 exact products per rounding, the fp32 instruction two;
    (ii) both agree on the non-PD flag."""
    X = correlated_x(T, C, rank, eps, seed=C + rank + int(eps * 100), massive=massive, mean_shift=mean)
    H = _h_of(ops, X)
    del X
    W = torch.randn(64, C, device="cuda")
    U_img, f_img, Hd = _chain(ops, H, W, "default")
    U_f32, f_f32, _ = _chain(ops, H, W, "fp32")
    assert f_img == f_f32 == 0  # damped: positive definite, and both say so
    U64 = fp64_chain(Hd)
    e_img, e_f32 = u_errors(U_img, U64), u_errors(U_f32, U64)
    print(f"\n[K3 corr] C={C} T={T} rank={rank} eps={eps} massive={massive} mean={mean}: image max/row/diag {e_img[0]:.2e} "
          f"{e_img[1]:.2e} {e_img[2]:.2e} | fp32 {e_f32[0]:.2e} {e_f32[1]:.2e} {e_f32[2]:.2e}")
    assert e_img[1] <= 1.25 * e_f32[1], (e_img, e_f32)
    assert e_img[0] <= 1.25 * e_f32[0], (e_img, e_f32)


def test_non_pd_flag_agrees_between_the_chains(ops):
    """(ii) on matrices that are NOT positive definite in fp32 -- gptq.py:321-323's bare except, the identity fallback:
    an indefinite perturbation well above the rounding level, applied in the bottom-right quadrant (seen by the image
    levels' Schur complement) and in the top-left one (seen by a leaf first)."""
    C = 4096
    X = correlated_x(2048, C, 64, 0.03, seed=11)
    H = _h_of(ops, X)
    del X
    W = torch.randn(64, C, device="cuda")
    for where in (C - 7, 5):
        Hb = H.clone()
        Hb[where, where] = -10.0 * float(Hb.diagonal().mean())  # stays negative after the 1 % damping
        for mode in ("default", "bf16x3", "fp32"):
            U, flag, _ = _chain(ops, Hb, W, mode)
            assert flag == 1, (where, mode)
            assert torch.equal(U, torch.eye(C, device="cuda")), (where, mode)  # U = I (gptq.py:322)


@pytest.mark.parametrize("massive,mean,eps", [(6, 0.0, 0.1), (0, 0.0, 0.3)])
def test_down_proj_ints_rate_on_a_correlated_hessian(ops, oracle, massive, mean, eps):
    """(iii) end to end at the width where all three image levels run: down_proj 4096 x 14336 Q4_K on a correlated Hessian,
    a 128-row slice through the oracle's column loop with the fp64 chain's U.  At this width the comparison's own noise
    floor -- two ORACLE runs whose U differ by 1e-7 relative, less than one fp32 rounding -- is already ~11 % of the ints
    (14336 dependent steps of error feedback through a correlated U; 1.6 % at 4096 iid), and the reference's precision (the
    all-fp32 chain) sits at 1.87 x that floor, the default chain at 1.72 x.  Asserted: the default chain is no further from
    the fp64 result than the all-fp32 chain (+ 5 % margin), and below 2 x the floor."""
    R, C, T = 4096, 14336, 16384
    X = correlated_x(T, C, C // 16, eps, seed=3, massive=massive, mean_shift=mean)
    H = _h_of(ops, X)
    del X
    g = torch.Generator(device="cuda").manual_seed(4)
    W0 = (torch.randn(R, C, device="cuda", generator=g) * 0.02).half().float()
    rows = slice(1024, 1152)
    res = {}
    for mode in ("default", "fp32"):
        with env(**CHAIN_MODES[mode]):
            Hc = H.clone()
            Wg = W0.clone()
            U, flag = ops.h_prepare(Hc, Wg, 0.01)
            assert int(flag.item()) == 0
            q = ops.gptq_quantize(Wg, U, 12, 128)[0]
        res[mode] = (q[rows].cpu().numpy(), U)
    Uo = fp64_chain(Hc)
    u_err = {m: u_errors(res[m][1], Uo) for m in res}
    Uo = Uo.cpu().numpy()
    Wo = W0[rows].cpu().numpy()
    _, oq, *_ = oracle.gptq_step(Wo, Uo.astype(np.float32), 12, block_size=128)
    rng = np.random.default_rng(0)
    Un = (Uo * (1.0 + 1e-7 * rng.standard_normal(Uo.shape))).astype(np.float32)
    _, nq, *_ = oracle.gptq_step(Wo, Un, 12, block_size=128)
    floor = float((nq != oq).mean())
    rate = {m: float((res[m][0] != oq).mean()) for m in res}
    print(f"\n[K3 corr] down_proj 4096x14336 Q4_K (massive={massive}, eps={eps}), rows 1024:1152: ints differ image "
          f"{rate['default']:.4%}, fp32 chain {rate['fp32']:.4%}, 1e-7 noise floor {floor:.4%}; U row-wise err image "
          f"{u_err['default'][1]:.2e} fp32 {u_err['fp32'][1]:.2e}")
    assert rate["default"] <= 1.05 * rate["fp32"] + 2e-3, (rate, floor)
    assert rate["default"] <= 2.0 * floor, (rate, floor)


# ----------------------------------------------------------------- K1: the four-wave form of the in-place SYRK
@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_h_accumulate_four_wave_form_is_bit_identical(ops, dt):
    """The in-place SYRK (syrk16_256w_kernel: 2 x 2 waves, 128 x 128 wave tiles, X read where it lies) against the other
    independent form in the tree, the operand-image kernel (option syrk_image: re-layout pass + syrk16_256e_kernel, 2 x 4
    waves): same k order per accumulator, so every Hessian is equal BIT FOR BIT wherever both add the same token ranges.
      * a single turn of the ring (T = 128, beta != 0): default == image, bit for bit;
      * two problems in one grid, T = 10240 >= 8192, beta != 0: the default cuts the last round of tiles into K-split
        units, which the image form does not have -- syrk_nosplit == image bit for bit, and the default within 5e-6 of
        fp64 (both problems);
      * per-sample blocks are refused on the image path: the blocked fold == the contiguous fold bit for bit, with the
        K-split (default) and without it (syrk_nosplit: hence == image as well).
    Every result is symmetric."""
    torch.manual_seed(41)
    shapes = [(2048, 5, 2048), (1280, 40, 256)]  # (C, blocks, tokens per block)
    Xl = [[(torch.randn(L, C, device="cuda") * torch.exp(torch.randn(C, device="cuda") * 0.5)).to(dt) for _ in range(nb)]
          for C, nb, L in shapes]
    Xc = [torch.cat(b) for b in Xl]
    H0 = [torch.randn(C, C, device="cuda") for C, _, _ in shapes]
    H0 = [h + h.T for h in H0]
    betas, alphas = [0.25, 0.5], [0.01, 0.02]

    def fold(blocked=True, **opts):
        with ops.options(**opts):
            Ha = [h.clone() for h in H0]
            ops.h_accumulate_grouped(Ha, Xc, betas, alphas)
            Hb = [h.clone() for h in H0]
            if blocked:
                ops.h_accumulate_grouped(Hb, Xl, betas, alphas)
            Hc = H0[1].clone()
            ops.h_accumulate(Hc, Xc[1][:128], 0.5, 0.125)   # one turn of the ring
        return Ha, Hb if blocked else None, Hc

    dflt, nosplit, image = fold(), fold(syrk_nosplit=1), fold(blocked=False, syrk_image=1)
    assert torch.equal(dflt[2], image[2])
    for k in range(2):
        assert torch.equal(nosplit[0][k], image[0][k]), k
        assert torch.equal(dflt[1][k], dflt[0][k]), k
        assert torch.equal(nosplit[1][k], nosplit[0][k]), k
        ref = betas[k] * H0[k].double() + alphas[k] * (Xc[k].double().T @ Xc[k].double())
        err = (dflt[0][k].double() - ref).abs().max().item() / ref.abs().max().item()
        print(f"\n[K1 four-wave] {dt} problem {k}: default vs fp64 {err:.2e}, default == image bit for bit: "
              f"{torch.equal(dflt[0][k], image[0][k])}")
        assert err <= 5e-6
    for h in dflt[0] + dflt[1] + [dflt[2]] + nosplit[0] + nosplit[1] + [nosplit[2]] + image[0] + [image[2]]:
        assert torch.equal(h, h.T)


# ----------------------------------------------------------------- stacked column loops (gq_gptq_quantize_stacked)
def _same(a, b):
    return all(torch.equal(x.view(torch.uint8) if x.dtype != torch.float16 else x.view(torch.int16),
                           y.view(torch.uint8) if y.dtype != torch.float16 else y.view(torch.int16)) for x, y in zip(a, b))


@pytest.mark.parametrize("q_type", [10, 11, 12, 13, 14])
@pytest.mark.parametrize("static_groups", [False, True])
def test_stacked_column_loop_equals_the_separate_calls(ops, q_type, static_groups):
    """Three matrices that share U, stacked by rows (320 + 64 + 128 rows, 768 columns), through gq_gptq_quantize_stacked:
    every output and the dequantized working copy equal the three gq_gptq_quantize calls BIT FOR BIT -- including the
    one place where the reference looks across the rows of a matrix: the middle matrix's first 256-column stripe holds ~1e-7
    values (no group of it is `valid` in any search iteration, quant_utils.py:250-252 skips them all for THAT Linear only),
    which a stacked call with ONE set of panel words gets wrong (checked: the un-segmented call differs there)."""
    torch.manual_seed(5 + q_type)
    C, rows = 768, [320, 64, 128]
    Ws = [torch.randn(r, C, device="cuda") * 0.02 for r in rows]
    Ws[1][:, :256] = torch.randn(64, 256, device="cuda") * 1e-7   # the first stripe: no error feedback reaches it
    U = torch.triu(torch.randn(C, C, device="cuda") * 0.01, 1) + torch.eye(C, device="cuda")
    kw = dict(block_size=128, static_groups=static_groups)
    sep, Wd = [], []
    for w in Ws:
        w = w.clone()
        sep.append(ops.gptq_quantize(w, U, q_type, **kw))
        Wd.append(w)
    Wf = torch.cat(Ws)
    ends = [320, 384, 512]
    st = ops.gptq_quantize(Wf, U, q_type, row_ends=ends, **kw)
    r0 = 0
    for k, r1 in enumerate(ends):
        assert _same([t[r0:r1] for t in st], sep[k]), f"matrix {k}"
        assert torch.equal(Wf[r0:r1], Wd[k])
        r0 = r1
    if q_type == 10 and not static_groups:  # the K-quant search where a skipped iteration's candidate would have won (Q2_K)
        Wu = torch.cat(Ws)
        un = ops.gptq_quantize(Wu, U, q_type, **kw)   # one matrix of 512 rows: the panel-wide `continue` sees all rows
        assert not _same([t[320:384] for t in un], sep[1]), "the per-matrix panel words were not needed here"
    with pytest.raises(Exception):
        ops.gptq_quantize(torch.cat(Ws), U, q_type, row_ends=[300, 384, 512], **kw)   # boundaries are multiples of 64
    with pytest.raises(Exception):
        ops.gptq_quantize(torch.cat(Ws), U, q_type, row_ends=[320, 384], **kw)        # the last one is R


def test_block_schedule_stacked_equals_unstacked_on_the_gpu(ops):
    """One Llama-shaped block (hidden 512: q 512, k / v 128 rows; gate / up 1024 rows) through BlockSchedule with and
    without stacking: identical results for every Linear, 4 column loops' worth of launches instead of 7."""
    import torch.nn as nn
    from gptq_gguf_toolkit_amd.block_schedule import BlockSchedule
    from gptq_gguf_toolkit_amd.gptq import GPTQ
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    torch.manual_seed(3)
    shapes = {"q": (512, 512), "k": (128, 512), "v": (128, 512), "o": (512, 512), "gate": (1024, 512), "up": (1024, 512),
              "down": (512, 1024)}
    w0 = {n: (torch.randn(r, c, device="cuda") * 0.02).half() for n, (r, c) in shapes.items()}
    xs, xo, xm = ([torch.randn(1, 256, 512, device="cuda").half() for _ in range(4)] for _ in range(3))
    xd = [torch.randn(1, 256, 1024, device="cuda").half() for _ in range(4)]
    outs = []
    for stack in (False, True):
        layers = {n: nn.Linear(c, r, bias=False, device="cuda", dtype=torch.float16) for n, (r, c) in shapes.items()}
        for n, l in layers.items():
            l.weight.data.copy_(w0[n])
        sch = BlockSchedule(layers, lambda l, n: GPTQ(l, block_size=128))
        sch.stack = stack
        for a, b, c, e in zip(xs, xo, xm, xd):
            for n in ("q", "k", "v"):
                sch.feed(n, a)      # one tensor: one Hessian, one factorisation
            sch.feed("o", b)
            for n in ("gate", "up"):
                sch.feed(n, c)
            sch.feed("down", e)
            sch.sample_done()
        res = sch.quantize({n: T.Q4_K for n in shapes})
        torch.cuda.synchronize()
        outs.append(({n: tuple(t.clone() for t in r) for n, r in res.items()}, {n: l.weight.data.clone() for n, l in layers.items()},
                     dict(sch.stats)))
    (r0, w_0, s0), (r1, w_1, s1) = outs
    for n in shapes:
        assert _same(r0[n], r1[n]), n
        assert torch.equal(w_0[n], w_1[n]), n
    assert s0.get("stacked", 0) == 0 and s1["stacked"] >= 3
    BlockSchedule.verify()


def test_ragged_folds_are_padded_to_whole_ring_turns(ops):
    """A handle fed ragged inputs (an MoE expert's data-dependent token counts) keeps them by reference, gathers them into
    its staging buffer with ONE launch when the fold is due (gq_h_stage_many) and pads the fold with zero rows to a
    multiple of 128 tokens: the fold then takes the kernel that reads X in place (no re-layout pass).  Zero
    tokens add exact zeros: H equals the operand-image path on the unpadded rows bit for bit, and fp64 to tolerance."""
    import torch.nn as nn
    from gptq_gguf_toolkit_amd.gptq import GPTQ
    torch.manual_seed(8)
    C = 512
    lin = nn.Linear(C, 64, bias=False, device="cuda", dtype=torch.float16)
    h = GPTQ(lin)
    xs = [torch.randn(1, t, C, device="cuda").half() for t in (100, 37, 300, 1)]
    for x in xs:
        h.update(x)
    assert len(h._rag) == 4 and h._staged == 0 and h._fill == 438   # kept by reference: one gather launch at the fold
    h.flush()
    assert not h._rag and h._buf.shape[0] >= 438 + 74
    X = torch.cat([x[0] for x in xs])
    with ops.options(syrk_image=1):
        ref = torch.zeros(C, C, device="cuda")
        ops.h_accumulate(ref, X, 0.0, 2.0 / 4)
    assert torch.equal(h.H, ref)
    d = 0.5 * (X.double().T @ X.double())
    assert (h.H.double() - d).abs().max().item() <= 3e-6 * d.abs().max().item()
    # a second, ragged fold on top (beta != 0), then one that needs no padding
    ys = [torch.randn(1, t, C, device="cuda").half() for t in (5, 250)]
    for y in ys:
        h.update(y)
    h.flush()
    h.update(torch.randn(1, 130, C, device="cuda").half()[:, :128].contiguous())
    h.flush()
    assert h.num_samples == 7 and torch.equal(h.H, h.H.T)
