"""-m gpu: the one-pass level build on the GPU.  gq_gptq_quantize_bands -- one column walk over row bands of different
K-quant types -- against the CPU oracle and against gq_gptq_quantize band by band (bit-exact), its refusals, the
handles (GPTQ.compute_levels) and the driver (Quantizer.quantize_levels) against ordinary one-level runs."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

Q2, Q3, Q4, Q5, Q6 = 10, 11, 12, 13, 14


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from gptq_gguf_toolkit_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u16(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def npy(t):
    return t.cpu().numpy()


def _problem(oracle, R, C, special_rows):
    """(W, U) as test_gptq_step_vs_oracle builds them; rows `special_rows` = (all-zero row, row with a constant 32-column
    group): the scale search's `const` branch and the eps clamp of a zero scale."""
    rng = np.random.default_rng(R + C)
    W0 = (rng.standard_normal((R, C)) * 0.02).astype(np.float16).astype(np.float32)
    zero_row, const_row = special_rows
    W0[zero_row] = 0.0
    W0[const_row, 32:64] = W0[const_row, 32]
    X = (rng.standard_normal((2 * C, C)) * np.exp(rng.standard_normal(C) * 0.5)).astype(np.float32)
    H = oracle.h_accumulate(np.zeros((C, C), np.float32), X, 0.0, 2.0 / 4)
    U, _, W1, bad = oracle.h_prepare(H, W0, 0.01)
    assert not bad
    return W1, U


def _ends(rows):
    return [int(e) for e in np.cumsum(rows)]


CASES = {
    # C = 512, block 128: the pair path (one launch walks both blocks of a 256-column group)
    "a_pair": (512, 128, [(Q2, 64), (Q3, 64), (Q4, 64), (Q5, 64), (Q6, 64)]),
    # C = 1280 crosses the 1024-column super-block: near updates and the chained far update; uneven, a repeated type
    "b_far": (1280, 128, [(Q4, 128), (Q6, 64), (Q2, 192), (Q4, 64), (Q3, 64)]),
    # block 64: no look-ahead, a trailing update after every block
    "c_block64": (512, 64, [(Q2, 64), (Q3, 64), (Q4, 64), (Q5, 64), (Q6, 64)]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_bands_equal_the_oracle_and_the_single_type_call(ops, oracle, case):
    C, block, spec = CASES[case]
    rows = [n for _, n in spec]
    ends, R = _ends(rows), sum(rows)
    # the special rows lie in the third band (Q4_K in a / c: G = 32, the constant group is one whole group; Q2_K in b)
    r_special = ends[1]
    W1, U = _problem(oracle, R, C, (r_special + 1, r_special + 5))
    W, Ud = dev(W1), dev(U)
    bands = [(e, t) for e, (t, _) in zip(ends, spec)]
    out = ops.gptq_quantize_bands(W, Ud, bands, block_size=block)
    torch.cuda.synchronize()
    assert len(out) == len(spec)
    r0 = 0
    for (t, n), r1, (q, d, s, dmin, m) in zip(spec, ends, out):
        Wd, oq, od, os_, odm, om = oracle.gptq_step(W1[r0:r1], U, t, block_size=block)
        tag = f"{case} band rows {r0}:{r1} type {t}"
        assert q.shape == (n, C) and s.shape == m.shape == os_.shape and d.shape == dmin.shape == (n, C // 256), tag
        assert np.array_equal(npy(q), oq), f"{tag}: {(npy(q) != oq).mean():.4%} ints differ"
        assert np.array_equal(u16(d), od) and np.array_equal(u16(dmin), odm), tag
        assert np.array_equal(npy(s), os_) and np.array_equal(npy(m), om), tag
        assert np.array_equal(npy(W[r0:r1]), Wd), tag
        # ... and gq_gptq_quantize on a clone of the band's rows alone
        Wc = dev(W1[r0:r1])
        alone = ops.gptq_quantize(Wc, Ud, t, block_size=block)
        for a, b in zip((q, d, s, dmin, m), alone):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), tag
        assert torch.equal(W[r0:r1], Wc), tag
        r0 = r1


def test_a_block_that_straddles_a_super_group_stays_inside_its_workspace(ops, oracle):
    """block_size 96 at C = 512: the block of columns 192 .. 287 crosses the 256-column super-group, is walked in two segments
    and lives in the block scratch.  The workspace the library asks for must hold that scratch: with exactly that many bytes,
    nothing behind them is written (the single-type call and the band walk), and the results are the oracle's."""
    from gptq_gguf_toolkit_amd import _cabi
    R, C, block = 128, 512, 96
    W1, U = _problem(oracle, R, C, (3, 70))
    Ud = dev(U)
    need = ops.workspace_bytes(_cabi.WS_GPTQ_QUANTIZE, R, C, 0, block)
    assert need >= 2 * R * block * 4  # the error buffer and the block scratch
    guard = 1 << 20
    for banded in (False, True):
        buf = torch.full((need + guard,), 0xAB, dtype=torch.uint8, device="cuda")
        W = dev(W1)
        if banded:
            outs = ops.gptq_quantize_bands(W, Ud, [(64, Q4), (128, Q6)], block_size=block, ws=buf[:need])
        else:
            outs = [ops.gptq_quantize(W, Ud, Q6, block_size=block, ws=buf[:need])]
        torch.cuda.synchronize()
        assert bool((buf[need:] == 0xAB).all()), f"banded={banded}: bytes behind the workspace were written"
        want = [(0, 64, Q4), (64, 128, Q6)] if banded else [(0, 128, Q6)]
        for (r0, r1, t), (q, d, s, dmin, m) in zip(want, outs):
            Wd, oq, od, os_, odm, om = oracle.gptq_step(W1[r0:r1], U, t, block_size=block)
            assert np.array_equal(npy(q), oq) and np.array_equal(u16(d), od) and np.array_equal(npy(s), os_)
            assert np.array_equal(u16(dmin), odm) and np.array_equal(npy(m), om) and np.array_equal(npy(W[r0:r1]), Wd)


def test_bad_band_tables_are_refused_before_anything_is_written(ops):
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()
    R, C, block = 256, 512, 128
    g = torch.Generator(device="cuda").manual_seed(5)
    W = torch.randn(R, C, device="cuda", generator=g) * 0.02
    U = torch.eye(C, device="cuda")
    W0 = W.clone()
    fill = 0xAB
    outs = {"q": torch.full((R * C,), fill, dtype=torch.uint8, device="cuda"),
            "d": torch.full((R * (C // 256) * 2,), fill, dtype=torch.uint8, device="cuda"),
            "s": torch.full((R * (C // 16),), fill, dtype=torch.uint8, device="cuda"),
            "dmin": torch.full((R * (C // 256) * 2,), fill, dtype=torch.uint8, device="cuda"),
            "m": torch.full((R * (C // 16),), fill, dtype=torch.uint8, device="cuda")}
    need = ops.workspace_bytes(_cabi.WS_GPTQ_QUANTIZE, R, C, 0, block)
    ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(bands, ws_bytes=need):
        tbl = (_cabi.Band * len(bands))(*[_cabi.Band(e, t) for e, t in bands])
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        return L.gq_gptq_quantize_bands(p(W), p(U), R, C, tbl, len(bands), block, None, p(outs["q"]), p(outs["d"]), p(outs["s"]),
                                        p(outs["dmin"]), p(outs["m"]), p(ws), ws_bytes, stream)

    good = [(64, Q4), (128, Q2), (256, Q6)]
    refused = {
        "unsorted": (([(128, Q4), (64, Q2), (256, Q6)],), "ascending"),
        "not a multiple of 64": (([(96, Q4), (256, Q2)],), "multiples of 64"),
        "last end != R": (([(64, Q4), (192, Q2)],), "last band ends"),
        "last end > R": (([(64, Q4), (320, Q2)],), "up to R"),
        "65 bands": (([(64 * (k + 1), Q4) for k in range(65)],), "65 bands"),
        "unknown type": (([(64, Q4), (256, 9)],), "unknown q_type 9"),
        "short workspace": ((good, need - 1), "workspace"),
    }
    for what, (args, msg) in refused.items():
        rc = call(*args)
        err = L.gq_last_error().decode()
        assert rc != 0 and msg in err, (what, rc, err)
    torch.cuda.synchronize()
    assert torch.equal(W, W0) and all(bool((t == fill).all()) for t in outs.values()) and bool((ws == fill).all())
    # the tensor-level entry point raises the same errors ...
    with pytest.raises(_cabi.GQError, match="ascending"):
        ops.gptq_quantize_bands(W, U, [(128, Q4), (64, Q2), (256, Q6)], block_size=block)
    with pytest.raises(_cabi.GQError, match="workspace"):
        ops.gptq_quantize_bands(W, U, good, block_size=block, ws=torch.empty(256, dtype=torch.uint8, device="cuda"))
    assert torch.equal(W, W0)
    # ... and the same table, accepted, works afterwards
    assert call(good) == 0
    torch.cuda.synchronize()
    assert not bool((outs["q"] == fill).all())


def test_compute_levels_equals_fifteen_fresh_handles(ops):
    """Three Linears on one input (rows 64 / 128 / 64, C = 512, bf16), five levels: one factorisation and one walk for
    the leader and the follower that shares its column sets; the third Linear has an all-zero weight column, so the
    leader's factor is not its factor: it is walked again with its own.  All equal quantize(t) of fresh handles."""
    from gptq_gguf_toolkit_amd.gptq import GPTQ
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    torch.manual_seed(21)
    C = 512
    lins = [torch.nn.Linear(C, r, bias=False).to(torch.bfloat16).cuda() for r in (64, 128, 64)]
    with torch.no_grad():
        lins[2].weight[:, 37] = 0
    xs = [(torch.randn(1, 96, C, device="cuda") * torch.exp(torch.randn(C, device="cuda") * 0.4)).to(torch.bfloat16)
          for _ in range(2)]
    kw = dict(rel_damp=0.01, block_size=128)
    hs = [GPTQ(l, **kw) for l in lins]
    for h in hs[1:]:
        h.shared_H_with, hs[0]._has_followers = hs[0], True
    for x in xs:
        for h in hs:
            h.update(x)
    for h in hs:
        h.quantization_pre_step()
    levels = list(T)
    got = GPTQ.compute_levels(hs, levels)
    assert set(got) == set(hs) and all(h.W is None and h._pending_mismatch is None for h in hs)
    for i, l in enumerate(lins):
        for t in levels:
            f = GPTQ(l, **kw)
            for x in xs:
                f.update(x)
            want = f.quantize(t)
            assert not f.issue_non_invertible
            for a, b in zip(got[hs[i]][t], want):
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (i, t.name)


# ---- the driver ----------------------------------------------------------------------------------------------------
def _drive(save_dir, how):
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd.quantizer import Quantizer
    os.makedirs(save_dir, exist_ok=True)
    model = tiny_llama().cuda()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    data = [([], {"input_ids": ids}) for ids in tiny_calib()]
    drv = Quantizer(model, data_loader=data, quantizable_modules=r".*layers.*((q|k|v|o|gate|up|down)_proj)$",
                    quantizer_kwargs=dict(rel_damp=0.01, block_size=128, act_order=False, quant_scale="absmax",
                                          static_groups=False, rmin=-1.0, rdelta=0.1, nstep=20, verbose=False),
                    pre_block_modules=["model.embed_tokens"], block_modules="model.layers",
                    post_block_modules=["lm_head"], quant_non_block_modules=False, device="cuda:0", save_dir=save_dir)
    t0 = time.perf_counter()
    how(drv)
    torch.cuda.synchronize()
    print(f"[levels] driver run into {os.path.basename(save_dir)}: {time.perf_counter() - t0:.2f} s")
    return model, before, dict(drv.schedule_stats)


def _tree(path):
    out = {}
    for n in sorted(os.listdir(path)):
        out[n] = torch.load(os.path.join(path, n, "data.pth"), weights_only=True)
    return out


def _rate(x, y):
    """Largest share of differing elements over the tensors of two data.pth dicts (q_type must agree)."""
    assert set(x) == set(y) and x["q_type"] == y["q_type"]
    worst = 0.0
    for k in x:
        if k == "q_type":
            continue
        assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape, k
        a = x[k].view(torch.int16) if x[k].dtype == torch.float16 else x[k]
        b = y[k].view(torch.int16) if y[k].dtype == torch.float16 else y[k]
        worst = max(worst, float((a != b).float().mean()))
    return worst


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from gptq_gguf_toolkit_amd.quant import DEFAULT_KEYS
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    from gptq_gguf_toolkit_amd import quantizer as qz
    root = tmp_path_factory.mktemp("levels")
    keep, keep_proc = os.environ.get("GQ_SAVE_SLOT_MB"), qz._Saver.USE_PROCESS
    os.environ["GQ_SAVE_SLOT_MB"] = "8"  # the tiny model's files: no 704 MB staging slots to pin per run
    levels = [T.Q2_K, T.Q4_K, T.Q6_K]
    r = {"levels": levels, "root": root}
    try:
        # the propagated level build writes through the default writer process; the five runs it is compared with write
        # from a thread (the same bytes; a writer process costs two seconds of start-up per run)
        r["lv"] = _drive(str(root / "lv"), lambda d: d.quantize_levels(levels, T.Q4_K))
        qz._Saver.USE_PROCESS = False
        for tag, t in (("q4_a", T.Q4_K), ("q4_b", T.Q4_K), ("q2", T.Q2_K), ("q6", T.Q6_K)):
            r[tag] = _drive(str(root / tag), lambda d, t=t: d.quantize({k: t for k in DEFAULT_KEYS}))
        r["none"] = _drive(str(root / "none"), lambda d: d.quantize_levels(levels, None))
    finally:
        qz._Saver.USE_PROCESS = keep_proc
        if keep is None:
            os.environ.pop("GQ_SAVE_SLOT_MB", None)
        else:
            os.environ["GQ_SAVE_SLOT_MB"] = keep
    # what the parent's path gives itself: two ordinary all-Q4_K runs, per module and for the model's weights
    a, b = _tree(root / "q4_a"), _tree(root / "q4_b")
    assert sorted(a) == sorted(b) and len(a) == 14
    r["self_rate"] = {n: _rate(a[n], b[n]) for n in a}
    r["self_weights"] = {n: float((p != dict(r["q4_b"][0].named_parameters())[n]).float().mean())
                         for n, p in r["q4_a"][0].named_parameters()}
    print("\n[levels] ordinary all-Q4_K run against itself, share of differing elements per module:",
          {n: v for n, v in r["self_rate"].items() if v} or "none (bit-identical)",
          "; weights:", {n: v for n, v in r["self_weights"].items() if v} or "bit-identical")
    return r


def test_driver_propagated_level_equals_its_ordinary_run(runs):
    """The Q4_K tree and the model after quantize_levels(propagate=Q4_K) against an ordinary all-Q4_K run: exactly what two
    ordinary runs give each other (measured in the fixture: bit-identical if they are, else no more than their rate)."""
    root = runs["root"]
    assert sorted(os.listdir(root / "lv")) == ["Q2_K", "Q4_K", "Q6_K"]
    want, got = _tree(root / "q4_a"), _tree(root / "lv" / "Q4_K")
    assert sorted(want) == sorted(got)
    for n in want:
        rate = _rate(got[n], want[n])
        print(f"    {n:44s} levels vs ordinary {rate:.4%}   ordinary vs ordinary {runs['self_rate'][n]:.4%}")
        assert rate <= runs["self_rate"][n], n
    ref = dict(runs["q4_a"][0].named_parameters())
    for n, p in runs["lv"][0].named_parameters():
        assert float((p != ref[n]).float().mean()) <= runs["self_weights"][n], n


def test_driver_other_levels_equal_block0_of_their_ordinary_runs(runs):
    """Block 0 sees the same inputs whatever is propagated: its Q2_K / Q6_K files equal the ordinary all-Q2_K / all-Q6_K
    runs (bound: the worst block-0 rate of the two ordinary Q4_K runs, zero when those are bit-identical)."""
    root = runs["root"]
    bound = max(v for n, v in runs["self_rate"].items() if ".layers.0." in n)
    for build in ("lv", "none"):
        for name, tag in (("Q2_K", "q2"), ("Q6_K", "q6"), ("Q4_K", "q4_a")):
            want, got = _tree(root / tag), _tree(root / build / name)
            assert sorted(want) == sorted(got)
            for n in want:
                if ".layers.0." in n:
                    assert _rate(got[n], want[n]) <= bound, (build, name, n)


def test_driver_propagate_none_leaves_the_model_untouched(runs):
    model, before, _ = runs["none"]
    assert sorted(os.listdir(runs["root"] / "none")) == ["Q2_K", "Q4_K", "Q6_K"]
    for n, p in model.named_parameters():
        assert torch.equal(p, before[n]), n
    changed = [n for n, p in runs["lv"][0].named_parameters() if not torch.equal(p, runs["lv"][1][n])]
    assert len(changed) == 14  # the propagated run replaced every quantized Linear's weight


def test_driver_factorises_no_more_than_a_single_level_run(runs):
    one = runs["q4_a"][2]
    for build in ("lv", "none"):
        st = runs[build][2]
        assert st["own_U"] <= one["own_U"] and st["reused_U"] >= one["reused_U"], (st, one)
        assert st["refactorised"] <= one["refactorised"] and st["syrk_launches"] == one["syrk_launches"], (st, one)
