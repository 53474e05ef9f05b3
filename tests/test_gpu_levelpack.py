"""-m gpu: gq_pack_bands -- the bands of one banded column walk as GGUF block bytes, every band into its own buffer, one
launch -- against the CPU oracle's packer on the gathered rows (never against the kernel under test), and against gq_pack
on the same slices.  Shapes are the smallest at which the kernel can go wrong: two blocks per row (the odd block of the 110-
and 210-byte types is 2-byte aligned), one block per row, a band that is not a whole turn of 32 blocks, 64 bands."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

Q2, Q3, Q4, Q5, Q6 = 10, 11, 12, 13, 14
TS = {Q2: 84, Q3: 110, Q4: 144, Q5: 176, Q6: 210}
GROUP = {Q2: 16, Q3: 16, Q4: 32, Q5: 32, Q6: 16}
CODES = {Q2: (0, 4), Q3: (-4, 4), Q4: (0, 16), Q5: (0, 32), Q6: (-32, 32)}      # [lo, hi) of the quantized values
SCALES = {Q2: (0, 16), Q3: (-32, 32), Q4: (0, 64), Q5: (0, 64), Q6: (-128, 128)}  # [lo, hi) of the group scales (and mins)
SPECIAL_FP16 = np.array([0x0000, 0x8000, 0x7BFF, 0xFBFF, 0x0001, 0x03FF, 0x8200, 0x3C00], np.uint16)  # zeros, max, subnormals, 1
GUARD = 64


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from gptq_gguf_toolkit_amd import ops as _ops
    return _ops


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()  # fp16 bit patterns travel as int16


def _inputs(spec, C, seed):
    """Stacked inputs of a band walk as it leaves them, random within each type's legal ranges: q [R, C] bytes, d / dmin
    [R, C / 256] fp16 bit patterns (any pattern, the special ones included: they pass through untouched), s / m in the
    concatenated per-band layout; dmin / m of Q3_K / Q6_K bands are 0xFF bytes (ignored).  -> numpy arrays and the table."""
    rng = np.random.default_rng(seed)
    R = sum(n for _, n in spec)
    q = np.empty((R, C), np.uint8)
    d = rng.integers(0, 1 << 16, (R, C // 256), dtype=np.uint16)
    dmin = rng.integers(0, 1 << 16, (R, C // 256), dtype=np.uint16)
    pick = rng.random((R, C // 256)) < 0.3
    d[pick] = rng.choice(SPECIAL_FP16, int(pick.sum()))
    dmin[~pick] = rng.choice(SPECIAL_FP16, int((~pick).sum()))
    s_parts, m_parts, bands, r0 = [], [], [], 0
    for t, n in spec:
        q[r0:r0 + n] = rng.integers(*CODES[t], (n, C)).astype(np.int8).view(np.uint8)
        s_parts.append(rng.integers(*SCALES[t], (n, C // GROUP[t])).astype(np.int8).view(np.uint8))
        if t in (Q3, Q6):
            dmin[r0:r0 + n] = 0xFFFF
            m_parts.append(np.full((n, C // GROUP[t]), 0xFF, np.uint8))
        else:
            m_parts.append(rng.integers(*SCALES[t], (n, C // GROUP[t])).astype(np.uint8))
        r0 += n
        bands.append((r0, t))
    s = np.concatenate([p.reshape(-1) for p in s_parts])
    m = np.concatenate([p.reshape(-1) for p in m_parts])
    return (q, d, s, dmin, m), s_parts, m_parts, bands


def _expected(oracle, arrays, s_parts, m_parts, spec, gathers):
    """oracle.pack per band, on that band's rows of all five tensors gathered with the band's index."""
    q, d, _, dmin, _ = arrays
    out, r0 = [], 0
    for k, (t, n) in enumerate(spec):
        idx = gathers[k] if gathers[k] is not None else np.arange(n)
        five = [q[r0:r0 + n][idx], d[r0:r0 + n][idx], s_parts[k][idx], dmin[r0:r0 + n][idx], m_parts[k][idx]]
        if t in (Q3, Q6):
            five[3], five[4] = None, None
        out.append(oracle.pack(t, *five))
        r0 += n
    return out


def _guarded(plan):
    """One buffer per band with GUARD bytes of 0xA5 on both sides -> (whole buffers, the views handed to the call)."""
    whole = [torch.full((nb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for *_, nb, _ in plan]
    return whole, [w[GUARD:GUARD + nb] for w, (*_, nb, _) in zip(whole, plan)]


def _run_and_check(ops, oracle, spec, C, gathers, seed):
    arrays, s_parts, m_parts, bands = _inputs(spec, C, seed)
    want = _expected(oracle, arrays, s_parts, m_parts, spec, gathers)
    stacked = tuple(dev(a) for a in arrays)
    before = [t.clone() for t in stacked]
    plan, _ = ops.pack_bands_plan(bands, C)
    whole, outs = _guarded(plan)
    srcs = [None if g is None else dev(g.astype(np.int32)) for g in gathers]
    got = ops.pack_bands(stacked, bands, outs, srcs)
    torch.cuda.synchronize()
    r0 = 0
    for k, ((t, n), g, w) in enumerate(zip(spec, got, want)):
        tag = f"band {k} type {t} rows {r0}:{r0 + n} gather {gathers[k] is not None}"
        assert tuple(g.shape) == w.shape == (n, C // 256 * TS[t]), tag
        assert np.array_equal(g.cpu().numpy(), w), f"{tag}: {(g.cpu().numpy() != w).mean():.4%} bytes differ from the oracle"
        assert bool((whole[k][:GUARD] == 0xA5).all()) and bool((whole[k][-GUARD:] == 0xA5).all()), f"{tag}: guard bytes written"
        # gq_pack on the same slices, gathered the way the converter gathers them
        idx = torch.arange(n, device="cuda") if gathers[k] is None else srcs[k].long()
        off = sum(rows * (C // GROUP[tt]) for tt, rows in spec[:k])
        nb = n * (C // GROUP[t])
        five = [stacked[0][r0:r0 + n][idx], stacked[1][r0:r0 + n][idx].view(torch.float16),
                stacked[2][off:off + nb].view(n, -1)[idx], stacked[3][r0:r0 + n][idx].view(torch.float16),
                stacked[4][off:off + nb].view(n, -1)[idx]]
        alone = ops.pack(t, *(five if t not in (Q3, Q6) else five[:3]))
        assert torch.equal(g, alone), f"{tag}: differs from gq_pack"
        r0 += n
    assert all(torch.equal(a, b) for a, b in zip(stacked, before)), "inputs were written"
    return got


def test_two_blocks_per_row_seven_bands_with_gathers(ops, oracle):
    from gptq_gguf_toolkit_amd.gguf_loader import rotary_row_dst
    spec = [(Q2, 64), (Q3, 64), (Q4, 128), (Q5, 64), (Q6, 128), (Q4, 64), (Q3, 64)]
    rot = rotary_row_dst("blk.0.attn_q.weight", 128, 2, 2, "cpu").numpy().astype(np.int64)  # 2 heads of 64 rows
    perm = np.random.default_rng(7).permutation(64)
    assert sum(n for _, n in spec) == 576
    _run_and_check(ops, oracle, spec, 512, [None, None, rot, None, rot, None, perm], seed=41)


def test_one_block_per_row(ops, oracle):
    _run_and_check(ops, oracle, [(Q6, 64), (Q2, 64)], 256, [None, None], seed=42)


def test_sixty_four_bands(ops, oracle):
    spec = [((Q2, Q3, Q4, Q5, Q6)[k % 5], 64) for k in range(64)]
    rng = np.random.default_rng(43)
    _run_and_check(ops, oracle, spec, 256, [rng.permutation(64) if k % 2 else None for k in range(64)], seed=43)


def test_output_of_a_real_walk(ops, oracle):
    """gq_gptq_quantize_bands on a [320, 512] problem with five types, then pack_bands of its per-band views (no copy: they
    are recognised as views into the walk's stacked buffers) against oracle.pack of the oracle's own walk per band."""
    rng = np.random.default_rng(320 + 512)
    R, C = 320, 512
    W0 = (rng.standard_normal((R, C)) * 0.02).astype(np.float16).astype(np.float32)
    W0[129] = 0.0
    W0[133, 32:64] = W0[133, 32]
    X = (rng.standard_normal((2 * C, C)) * np.exp(rng.standard_normal(C) * 0.5)).astype(np.float32)
    H = oracle.h_accumulate(np.zeros((C, C), np.float32), X, 0.0, 2.0 / 4)
    U, _, W1, bad = oracle.h_prepare(H, W0, 0.01)
    assert not bad
    types = [Q2, Q3, Q4, Q5, Q6]
    bands = [(64 * (k + 1), t) for k, t in enumerate(types)]
    res = ops.gptq_quantize_bands(dev(W1), dev(U), bands, block_size=128)
    got = ops.pack_bands(res, bands)
    torch.cuda.synchronize()
    for k, t in enumerate(types):
        _, oq, od, os_, odm, om = oracle.gptq_step(W1[64 * k:64 * (k + 1)], U, t, block_size=128)
        want = oracle.pack(t, oq, od, os_, odm, om) if t not in (Q3, Q6) else oracle.pack(t, oq, od, os_)
        assert np.array_equal(got[k].cpu().numpy(), want), f"band {k} type {t}"
        assert torch.equal(got[k], ops.pack(t, *(res[k] if t not in (Q3, Q6) else res[k][:3]))), f"band {k} type {t}"


def test_bad_calls_are_refused_before_anything_is_written(ops):
    from gptq_gguf_toolkit_amd import _cabi
    L = _cabi.lib()
    R, C = 192, 512
    spec = [(Q4, 64), (Q3, 64), (Q6, 64)]
    arrays, _, _, good = _inputs(spec, C, seed=44)
    q, d, s, dmin, m = (dev(a) for a in arrays)
    plan, _ = ops.pack_bands_plan(good, C)
    fill = 0xA5
    outs = [torch.full((nb + 16,), fill, dtype=torch.uint8, device="cuda") for *_, nb, _ in plan]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = ctypes.c_void_p

    def call(bands, C=C, R=R, out_ptrs=None):
        n = len(bands)
        tbl = (_cabi.Band * max(n, 1))(*[_cabi.Band(e, t) for e, t in bands])
        ptrs = out_ptrs if out_ptrs is not None else [o.data_ptr() for o in outs]
        op = (vp * max(n, 1))(*(ptrs + [ptrs[-1]] * n)[:n])
        return L.gq_pack_bands(vp(q.data_ptr()), vp(d.data_ptr()), vp(s.data_ptr()), vp(dmin.data_ptr()), vp(m.data_ptr()), R, C,
                               tbl, n, op, None, stream)

    p = [o.data_ptr() for o in outs]
    refused = {
        "unsorted": (dict(bands=[(128, Q4), (64, Q3), (192, Q6)]), _cabi_status("BAD_SHAPE"), "ascending"),
        "not a multiple of 64": (dict(bands=[(96, Q4), (192, Q3)]), _cabi_status("BAD_SHAPE"), "multiples of 64"),
        "last end != R": (dict(bands=[(64, Q4), (128, Q3)]), _cabi_status("BAD_SHAPE"), "last band ends"),
        "last end > R": (dict(bands=[(64, Q4), (256, Q3)]), _cabi_status("BAD_SHAPE"), "up to R"),
        "65 bands": (dict(bands=[(64 * (k + 1), Q4) for k in range(65)]), _cabi_status("BAD_SHAPE"), "65 bands"),
        "no bands": (dict(bands=[]), _cabi_status("BAD_SHAPE"), "0 bands"),
        "unknown type": (dict(bands=[(64, Q4), (192, 9)]), _cabi_status("BAD_TYPE"), "unknown q_type 9"),
        "C % 256": (dict(bands=good, C=384), _cabi_status("BAD_SHAPE"), "C % 256"),
        "NULL out": (dict(bands=good, out_ptrs=[p[0], 0, p[2]]), _cabi_status("NULL"), "band 1: out is NULL"),
        "misaligned out": (dict(bands=good, out_ptrs=[p[0], p[1], p[2] + 8]), _cabi_status("BAD_SHAPE"), "band 2: out not 16-byte aligned"),
    }
    for what, (kw, status, msg) in refused.items():
        rc = call(**kw)
        err = L.gq_last_error().decode()
        assert rc == status and msg in err, (what, rc, err)
    torch.cuda.synchronize()
    assert all(bool((o == fill).all()) for o in outs)
    # the tensor-level entry point: the plan refuses a bad table as a ValueError, the library's refusals are GQError
    with pytest.raises(ValueError, match="ascending"):
        ops.pack_bands((q, d, s, dmin, m), [(128, Q4), (64, Q3), (192, Q6)])
    with pytest.raises(_cabi.GQError, match="16-byte aligned"):
        ops.pack_bands((q, d, s, dmin, m), good, [outs[0][:plan[0][4]], outs[1][:plan[1][4]], outs[2][8:8 + plan[2][4]]])
    assert all(bool((o == fill).all()) for o in outs)
    # ... and the same table, accepted, works afterwards
    assert call(good) == 0
    torch.cuda.synchronize()
    assert all(not bool((o[:nb] == fill).all()) and bool((o[nb:] == fill).all()) for o, (*_, nb, _) in zip(outs, plan))


def _cabi_status(name):
    """GQ_E_* of include/gptq_gguf.h."""
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "gptq_gguf.h")).read()
    return int(re.search(rf"GQ_E_{name}\s*=?\s*(-?\d+)", text).group(1))
