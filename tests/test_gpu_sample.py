"""gq_sample_logits on the GPU against the fp64 statement of its contract (tests/sample_oracle.py).  The inputs are built so
that the expected token is exact: top_p and every u sit in the middle of a gap between prefix masses that is far wider than
the fp32 error of a 1024-term sum (about 1024 * 2^-24 * a small constant ~ 1e-4 relative), so the margins asserted here
(1e-3 for top_p, a probability of 2e-3 -- a half-interval of 1e-3 -- for u) are derived from the number format, not measured."""
import numpy as np
import pytest

import sample_oracle as so

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
TOP_KS, TEMPS = (1, 7, 40, 50, 1024), (0.3, 0.8, 1.0, 2.0)


def make_logits(V, dtype, seed, scale=3.0):
    """3 randn rounded to fp16, cast to `dtype` -> (the [V] tensor on the CPU, its exact values as float32 numpy)."""
    g = torch.Generator().manual_seed(seed)
    x = (scale * torch.randn(V, generator=g)).to(torch.float16).to(dtype)
    return x, x.float().numpy()


def rows_on_device(x, B, pad=0):
    """B copies of the row x as a [B, V] view with row stride V + pad (the pad holds NaN: it must never be read)."""
    buf = torch.full((B, x.numel() + pad), float("nan"), dtype=x.dtype)
    buf[:, :x.numel()] = x
    return buf.cuda()[:, :x.numel()]


def midpoint_top_p(z, top_k, t):
    """top_p in the middle of the widest gap between consecutive prefix masses inside [0.85, 0.95] -> (top_p, half gap).
    A flat distribution (V >= 512 candidates at temperature 2: every token there weighs about 1e-3, which is an upper bound of
    the widest gap) has no gap of twice the 1e-3 margin in that window; then -- and only then -- the gap is the nearest one
    BELOW the window that has the margin, so the margin the callers assert stays 1e-3 for every case."""
    tab = so.table(z, top_k, 1.0, t)
    mass = tab["cdf"] / tab["cdf"][-1]
    pts = np.concatenate(([0.85], mass[(mass > 0.85) & (mass < 0.95)], [0.95]))
    i = int(np.argmax(np.diff(pts)))
    if pts[i + 1] - pts[i] < 2e-3:
        pts = np.concatenate(([0.0], mass[mass < 0.85], [0.85]))
        i = int(np.nonzero(np.diff(pts) >= 2e-3)[0][-1])
    return float(np.float32((pts[i] + pts[i + 1]) / 2)), float(pts[i + 1] - pts[i]) / 2


def midpoint_draws(z, top_k, top_p, t, p_min=2e-3):
    """For every rank of the nucleus with probability >= p_min: u in the middle of its CDF interval -> (u float32, ids)."""
    tab = so.table(z, top_k, top_p, t)
    n = tab["n"]
    cdf = np.concatenate(([0.0], tab["cdf"][:n])) / tab["cdf"][n - 1]
    ranks = np.nonzero(np.diff(cdf) >= p_min)[0]
    assert ranks.size >= 1
    return ((cdf[ranks] + cdf[ranks + 1]) / 2).astype(np.float32), tab["ids"][ranks]


@pytest.mark.parametrize("V", [1, 37, 512, 513, 1000])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_midpoint_draws_return_the_oracle_token(dt, V):
    from gptq_gguf_toolkit_amd import ops
    x, z = make_logits(V, DTYPES[dt], seed=1000 + V)
    checked = 0
    for top_k in TOP_KS:
        for t in TEMPS:
            t32 = float(np.float32(t))
            top_p, half = midpoint_top_p(z, top_k, t32)
            assert half >= 1e-3, (top_k, t, half)
            u, want = midpoint_draws(z, top_k, top_p, t32)
            for pad in (0, 3):
                got = ops.sample_logits(rows_on_device(x, len(u), pad), torch.from_numpy(u).cuda(), top_k, top_p, t)
                assert got.dtype == torch.int64 and got.tolist() == want.tolist(), (top_k, t, pad)
                # the oracle's own draw agrees with the table it was built from
            assert so.sample(z, u[0], top_k, top_p, t32) == want[0]
            checked += len(u)
    print(f"{dt} V={V}: {checked} midpoint draws")


@pytest.mark.parametrize("dt,V,top_k,t", [("f16", 1000, 50, 2.0), ("f32", 513, 1024, 2.0), ("bf16", 3000, 200, 1.0)])
def test_grid_of_draws_inverts_the_cdf(dt, V, top_k, t):
    """u_i = (i + 0.5) / 4096 on 4096 copies of a row: an exact inversion gives every nucleus token 4096 p draws to within 1,
    the fp32 error of the prefix sums (1e-4 * 4096) adds less than 1: |count - 4096 p| <= 2, and no other id appears."""
    from gptq_gguf_toolkit_amd import ops
    B = 4096
    x, z = make_logits(V, DTYPES[dt], seed=7)
    t32 = float(np.float32(t))
    top_p, half = midpoint_top_p(z, top_k, t32)
    assert half >= 1e-3
    tab = so.table(z, top_k, top_p, t32)
    n = tab["n"]
    p = tab["w"][:n] / tab["cdf"][n - 1]
    u = ((torch.arange(B, dtype=torch.float64) + 0.5) / B).float().cuda()
    got = ops.sample_logits(rows_on_device(x, B), u, top_k, top_p, t).cpu().numpy()
    assert set(got.tolist()) <= set(tab["ids"][:n].tolist())
    count = np.array([(got == i).sum() for i in tab["ids"][:n]])
    worst = float(np.abs(count - B * p).max())
    print(f"{dt} V={V} top_k={top_k}: nucleus of {n}, worst |count - 4096 p| = {worst:.3f}")
    assert worst <= 2


@pytest.mark.parametrize("V,top_k", [(300, 40), (3000, 40), (3000, 1024), (128256, 1000)])
def test_ties_at_the_kth_place_go_to_the_lowest_indices(V, top_k):
    """Five distinct values only, so the K-th place falls inside a run of equal logits; a nearly flat distribution and a grid
    of u reach every candidate: the set of returned ids is the oracle's candidate set."""
    from gptq_gguf_toolkit_amd import ops
    g = torch.Generator().manual_seed(V + top_k)
    x = torch.tensor([-1.5, -0.0, 0.0, 0.25, 2.0], dtype=torch.float16)[torch.randint(0, 5, (V,), generator=g)]
    z = x.float().numpy()
    ids = so.order(z)[:top_k]
    assert z[ids[-1]] == z[so.order(z)[top_k]]  # the boundary is inside a tie
    B = 4096
    u = ((torch.arange(B, dtype=torch.float64) + 0.5) / B).float().cuda()
    got = ops.sample_logits(rows_on_device(x, B, pad=1), u, top_k, 1.0, 1e4)
    assert set(got.tolist()) == set(ids.tolist())


def test_argmax_takes_the_lowest_index_and_needs_no_u():
    from gptq_gguf_toolkit_amd import ops
    for dt in DTYPES.values():
        for V in (1, 5, 1000, 128256):
            x = torch.stack([make_logits(V, dt, seed=s)[0] for s in range(3)])
            want = []
            for r in range(3):  # the maximum up to three times, its first place late in a 16-byte group
                where = sorted({(11 * (r + 1)) % V, V // 2, V - 1})
                x[r, where] = 20.0
                want.append(where[0])
            assert want == [so.sample(x[r].float().numpy(), 0.0, 40, 1.0, 0.0) for r in range(3)]
            buf = torch.zeros(3, V + 5, dtype=dt)
            buf[:, :V] = x
            got = ops.sample_logits(buf.cuda()[:, :V], None, 40, 0.9, 0.0)
            assert got.tolist() == want
            # top_k = 1 is the same token whatever u says
            u = torch.tensor([0.0, 0.5, 0.999], device="cuda")
            assert ops.sample_logits(buf.cuda()[:, :V], u, 1, 1.0, 0.7).tolist() == want
    x = torch.tensor([[-0.0, 0.0, -1.0], [0.0, -0.0, -1.0]], dtype=torch.float32).cuda()
    assert ops.sample_logits(x, None, 3, 1.0, 0.0).tolist() == [0, 0]  # -0 == +0


def test_bad_rows_give_minus_one_and_leave_their_neighbours_alone():
    from gptq_gguf_toolkit_amd import ops
    for dt in DTYPES.values():
        for V in (9, 2000):
            x, z = make_logits(V, dt, seed=3)
            rows = x.repeat(7, 1)
            rows[1, V - 1] = float("nan")
            rows[3, :] = float("-inf")
            rows[5, V // 2] = float("inf")
            for t in (0.0, 0.9):
                t32 = float(np.float32(t))
                u0 = midpoint_draws(z, 5, 1.0, t32)[0][0] if t else np.float32(0.5)
                got = ops.sample_logits(rows.cuda(), torch.full((7,), float(u0)).cuda(), 5, 1.0, t).tolist()
                good = so.sample(z, u0, 5, 1.0, t32)
                assert got == [good, -1, good, -1, good, -1, good]


def test_minus_infinity_candidates_are_never_drawn():
    from gptq_gguf_toolkit_amd import ops
    x = torch.full((20,), float("-inf"), dtype=torch.float16)
    x[[2, 5, 11, 12, 19]] = torch.tensor([0.5, 1.0, 0.25, 0.75, 0.0], dtype=torch.float16)
    z = x.float().numpy()
    B = 257
    u = (torch.arange(B, dtype=torch.float64) / (B - 1)).float()
    u[-1] = 1 - 2.0 ** -24
    got = ops.sample_logits(rows_on_device(x, B), u.cuda(), 10, 1.0, 1.0).tolist()
    assert set(got) == {2, 5, 11, 12, 19}
    assert got[-1] == so.sample(z, u[-1].item(), 10, 1.0, 1.0) == 19  # the last candidate with a positive weight
    assert got[0] == 5


def test_one_row_of_a_real_vocabulary():
    """V = 128256 does not fit LDS: the select re-reads the row.  fp16, top_k = 1024, five ranks spread over those with a
    probability of at least 2e-3; the row starts 2 bytes past a 16-byte boundary."""
    from gptq_gguf_toolkit_amd import ops
    V = 128256
    x, z = make_logits(V, torch.float16, seed=11)
    top_p, half = midpoint_top_p(z, 1024, 1.0)
    assert half >= 1e-3
    u, want = midpoint_draws(z, 1024, top_p, 1.0)
    pick = np.unique(np.linspace(0, len(u) - 1, 5).astype(int))
    assert len(pick) == 5
    buf = torch.zeros(5, V + 9, dtype=torch.float16)
    buf[:, 1:V + 1] = x
    rows = buf.cuda()[:, 1:V + 1]
    got = ops.sample_logits(rows, torch.from_numpy(u[pick]).cuda(), 1024, top_p, 1.0)
    assert got.tolist() == want[pick].tolist()
    again = ops.sample_logits(rows, torch.from_numpy(u[pick]).cuda(), 1024, top_p, 1.0)
    assert torch.equal(got, again)


def test_python_layer_refusals_on_the_device():
    from gptq_gguf_toolkit_amd import ops
    from gptq_gguf_toolkit_amd._cabi import GQError
    x = torch.zeros(2, 8, device="cuda")
    u = torch.zeros(2, device="cuda")
    for kw in (dict(top_k=0), dict(top_k=1025), dict(top_k=4, top_p=0.0), dict(top_k=4, top_p=1.5),
               dict(top_k=4, temperature=-1.0), dict(top_k=4, temperature=float("nan"))):
        with pytest.raises(GQError):
            ops.sample_logits(x, u, **kw)
    with pytest.raises(GQError):
        ops.sample_logits(x, None, 4, 1.0, 1.0)
    with pytest.raises(GQError):
        ops.sample_logits(x.expand(4, 2, 8)[:, 0], torch.zeros(4, device="cuda"), 4)  # row stride 0 < V
    with pytest.raises(GQError):
        ops.sample_logits(x.long(), u, 4)
