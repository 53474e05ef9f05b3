"""The grouped MoE kernels on the GPU at real expert counts: gq_linear_packed_experts (K25) at E = 5, 8, 9, 64, 255 and 256,
gq_gemv_packed_experts (K24) at E = 8, 64, 256 and 65535, and PackedExperts at (E, K) = (8, 2) and (64, 8).  The other MoE files
run with three or four experts, where linear_packed_experts_kernel's wave-wide search for a workgroup's (expert, token tile) never
leaves lane 0; the pair sets of tests/moe_cases.py put tiles into the other lanes, behind empty experts, into lane 63's last slot
and clamped read, and leave workgroups of the grid without a tile (tests/test_moe_cases_cpu.py pins all of that on the host).

Every written row is compared bit for bit with the single-matrix kernel on the expert's slice, in one torch.equal over [P, R];
rows of masked pairs keep the fill; guards, a second call and the binding as in test_gpu_moe_prefill.py / test_gpu_moe_gemv.py;
fp64 within test_gpu_qgemm.py's bound.  R = 40 (one row tile) and 130 (two, 2-byte stores), C = 512 for the GEMM; the GEMV's
shapes are test_gpu_moe_gemv.py's."""
import pytest

import moe_cases as M
from moe_cases import ALL8, BF16, F16, NL, Q2, Q3, Q4, Q5, Q6, Q8, XS
from test_gpu_decode import bits
from test_gpu_moe_gemv import SHAPES
from test_gpu_moe_gemv import raw_call as raw_gemv
from test_gpu_moe_prefill import raw_call as raw_gemm
from test_gpu_qgemm import FILL, guarded_y, guards_intact, ops  # noqa: F401
from test_moe_prefill_cpu import route_by_sort

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = 512
ROWS = (40, 130)
NAME = {10: "q2", 11: "q3", 12: "q4", 13: "q5", 14: "q6", 8: "q8", NL: "iq4nl", XS: "iq4xs"}
ident = lambda cases: [f"{c[0]}-{NAME[c[1]]}-{str(c[2])[6:]}" for c in cases]  # noqa: E731


# ------------------------------------------------------------------------------------------------ a, b: the grouped GEMM
def gemm_case(ops, name, t, dt, wide=None):  # noqa: F811
    """One pair set through gq_moe_route and gq_linear_packed_experts for both row counts: the route is torch's stable sort,
    every written row is expected_rows' bit for bit, every other row keeps the fill, nothing outside y is written, a second call
    and the binding give the same bits."""
    E = M.EXPECT[name]["E"]
    x_rows, ppr, ids = M.PAIR_SETS[name]()
    P = len(ids)
    assert (P >= 128 * E) == M.EXPECT[name]["wide"] and (wide is None or wide == (P >= 128 * E and t in M.WIDE_OK))
    pe = torch.tensor(ids, dtype=torch.int32, device="cuda")
    route = ops.moe_route(pe, E)
    want_start, want_order = route_by_sort(pe, E)
    assert torch.equal(route[0], want_start) and torch.equal(route[1], want_order), name
    x = M.inputs(x_rows, C, dt, t)
    for R in ROWS:
        src = M.stacked(ops, t, E, R, C)
        buf, y = guarded_y(P, R, dt)
        assert raw_gemm(t, src, R, x, ppr, route, y, n_experts=E) == 0
        want, written = M.expected_rows(ops, t, src, E, ids, x, ppr)
        assert int(written.sum()) == sum(0 <= e < E for e in ids) > 0
        diff = (bits(y) != bits(want))[written]
        assert not bool(diff.any()), (name, R, f"{int(diff.any(-1).sum())} of {int(written.sum())} written rows differ")
        assert bool((bits(y)[~written] == FILL).all()), (name, R, "a skipped pair's row was written")
        assert guards_intact(buf), (name, R, "written outside [y, y + P * R * 2)")
        assert bool(torch.isfinite(y[written]).all()) and float(y[written].float().abs().max()) > 0
        buf2, y2 = guarded_y(P, R, dt)
        assert raw_gemm(t, src, R, x, ppr, route, y2, n_experts=E) == 0
        assert torch.equal(bits(y2), bits(y)), (name, R, "two calls differ")
        got = ops.linear_packed_experts(t, src, E, R, x, route, ppr)  # the binding: the same call
        assert torch.equal(bits(got)[written], bits(y)[written]), (name, R)


@pytest.mark.parametrize("name,t,dt", M.GEMM_NARROW, ids=ident(M.GEMM_NARROW))
def test_narrow_tile_every_pair_is_linear_packed_on_its_experts_slice(ops, name, t, dt):  # noqa: F811
    """The 128-token tile (P < 128 E): tiles in lanes 0 and 1 (mixtral, skewed8, masked8, tiny5 with the clamp in lane 1), in
    lanes 0 .. 15 (qwen64), one tile per (lane, slot) of the wave (each256) and two tiles in lane 63's last slot, E = 256 and
    E = 255 (last256, last255)."""
    gemm_case(ops, name, t, dt, wide=False)


@pytest.mark.parametrize("name,t,dt", M.GEMM_WIDE, ids=ident(M.GEMM_WIDE))
def test_wide_tile_gives_the_bits_of_linear_packed(ops, name, t, dt):  # noqa: F811
    """P >= 128 E: the 256-token tile for the types that have it, the 128-token one for Q4_K and IQ4_XS.  The reference,
    linear_packed with one expert's tokens, runs its 128-token tile at these row counts: equal bits across the two widths and the
    two kernels.  wide8: eight tiles in lanes 0 and 1, cuts at 1, 16, 17 and 88 tokens, 134 masked pairs; wide9: expert 8 in
    lane 2."""
    gemm_case(ops, name, t, dt, wide=t in M.WIDE_OK)


@pytest.mark.parametrize("name,wide", [("switch1023", False), ("switch1024", True)])
def test_the_width_switch_at_128_e(ops, name, wide):  # noqa: F811
    """E = 8: P = 1023 is the last call of the 128-token tile, P = 1024 the first of the 256-token one; the same distribution,
    the same reference."""
    gemm_case(ops, name, Q6, F16 if wide else BF16, wide=wide)


# ------------------------------------------------------------------------------------------------ c: the grouped GEMM, fp64
FP64 = [("skewed8", Q3, F16), ("qwen64", XS, BF16), ("each256", NL, F16), ("wide8", Q6, BF16)]


@pytest.mark.parametrize("name,t,dt", FP64, ids=ident(FP64))
def test_grouped_gemm_against_fp64(ops, name, t, dt):  # noqa: F811
    """test_gpu_qgemm.py's bound per element of every written row: u |y64| + C 2^-23 (|x| |Wd|^T) + 2^-25, u = 2^-11 fp16 /
    2^-8 bf16.  [130, 512] per expert."""
    R, E = 130, M.EXPECT[name]["E"]
    x_rows, ppr, ids = M.PAIR_SETS[name]()
    pe = torch.tensor(ids, dtype=torch.int32, device="cuda")
    src = M.stacked(ops, t, E, R, C)
    x = M.inputs(x_rows, C, dt, t)
    y = ops.linear_packed_experts(t, src, E, R, x, ops.moe_route(pe, E), ppr)
    y64, bound = M.fp64_rows(ops, t, src, E, R, C, ids, x, ppr, dt)
    written = (pe >= 0) & (pe < E)
    err = (y.double() - y64).abs()[written]
    worst = float((err / bound[written]).max())
    print(f"{name} E={E} q_type {t} {dt}: max err / bound = {worst:.3f}")
    assert bool(torch.isfinite(y[written]).all()) and float(y[written].float().abs().max()) > 0
    assert bool((err <= bound[written]).all()), f"max err / bound = {worst}"


# ------------------------------------------------------------------------------------------------ d: the grouped GEMV
def gemv_sets():
    """name -> (E, x_rows, pairs_per_row, ids): P <= 64 pairs."""
    ids256 = [0, 255] + (torch.randperm(254, generator=torch.Generator().manual_seed(31))[:62] + 1).tolist()
    ids256 = [ids256[i] for i in torch.randperm(64, generator=torch.Generator().manual_seed(32)).tolist()]
    return {"E8-T16-K2": (8, 16, 2, M._top_k(16, 8, 2, 33)),          # the decode step of Mixtral at the GEMV's largest T
            "E64-T8-K8": (64, 8, 8, M._top_k(8, 64, 8, 34)),           # P = 64, the maximum
            "E256-P64": (256, 64, 1, ids256)}                          # 64 different experts, 0 and 255 among them


GEMV = [(n, s, ALL8[i % 8], (F16, BF16)[(i + i // 8) % 2]) for i, (n, s) in enumerate((n, s) for n in gemv_sets() for s in SHAPES)]


def gemv_case(ops, t, dt, E, R, Cg, x_rows, ppr, ids, binding=True):  # noqa: F811
    src = M.stacked(ops, t, E, R, Cg)
    x = M.inputs(x_rows, Cg, dt, t)
    pe = torch.tensor(ids, dtype=torch.int32, device="cuda")
    buf, y = guarded_y(len(ids), R, dt)
    assert raw_gemv(t, src, R, Cg, x, pe, ppr, y, E=E) == 0
    want, written = M.gemv_rows(ops, t, src, E, ids, x, ppr)
    assert int(written.sum()) == sum(0 <= e < E for e in ids) > 0
    diff = (bits(y) != bits(want))[written]
    assert not bool(diff.any()), (E, R, Cg, f"{int(diff.any(-1).sum())} of {int(written.sum())} written rows differ")
    assert bool((bits(y)[~written] == FILL).all()), (E, R, Cg, "a skipped pair's row was written")
    assert guards_intact(buf), (E, R, Cg, "written outside [y, y + P * R * 2)")
    assert bool(torch.isfinite(y[written]).all()) and float(y[written].float().abs().max()) > 0
    buf2, y2 = guarded_y(len(ids), R, dt)
    assert raw_gemv(t, src, R, Cg, x, pe, ppr, y2, E=E) == 0
    assert torch.equal(bits(y2), bits(y)), (E, R, Cg, "two calls differ")
    got = ops.gemv_packed_experts(t, src, E, R, x, pe, ppr)  # the binding: the same call
    assert torch.equal(bits(got)[written], bits(y)[written])
    return src, x, pe, y


@pytest.mark.parametrize("name,shape,t,dt", GEMV, ids=[f"{c[0]}-R{c[1][0]}-C{c[1][1]}-{NAME[c[2]]}-{str(c[3])[6:]}" for c in GEMV])
def test_grouped_gemv_every_pair_is_gemv_packed_on_its_experts_slice(ops, name, shape, t, dt):  # noqa: F811
    E, x_rows, ppr, ids = gemv_sets()[name]
    if ppr > 1:
        assert all(len(set(ids[i:i + ppr])) == ppr for i in range(0, len(ids), ppr)), "distinct experts per token"
    if name == "E256-P64":
        assert len(set(ids)) == 64 and {0, 255} <= set(ids)
    gemv_case(ops, t, dt, E, shape[0], shape[1], x_rows, ppr, ids)


@pytest.mark.parametrize("t,dt", [(Q8, F16), (Q4, BF16)], ids=["q8", "q4"])
def test_grouped_gemv_at_its_largest_expert_count(ops, t, dt):  # noqa: F811
    """E = 65535, the largest grid: expert 65534 is the last workgroup row; id 65535 = E is the masked pair, as is -1."""
    E, R, Cg = 65535, 18, 256
    gemv_case(ops, t, dt, E, R, Cg, 3, 2, [0, 65534, 65535, 3, 65534, -1])


@pytest.mark.parametrize("t,dt", [(Q5, F16), (NL, BF16)], ids=["q5", "iq4nl"])
def test_grouped_gemv_against_fp64(ops, t, dt):  # noqa: F811
    """test_gpu_qgemv.py's bound (the one-Linear bound of fp64_rows) for E = 64, P = 64, [40, 4352]."""
    E, x_rows, ppr, ids = gemv_sets()["E64-T8-K8"]
    R, Cg = 40, 4352
    src = M.stacked(ops, t, E, R, Cg)
    x = M.inputs(x_rows, Cg, dt, t)
    y = ops.gemv_packed_experts(t, src, E, R, x, torch.tensor(ids, dtype=torch.int32, device="cuda"), ppr)
    y64, bound = M.fp64_rows(ops, t, src, E, R, Cg, ids, x, ppr, dt)
    err = (y.double() - y64).abs()
    worst = float((err / bound).max())
    print(f"E=64 P=64 q_type {t} {dt}: max err / bound = {worst:.3f}")
    assert bool(torch.isfinite(y).all()) and float(y.float().abs().max()) > 0
    assert bool((err <= bound).all()), f"max err / bound = {worst}"


# ------------------------------------------------------------------------------------------------ e, f: the module
H, I = 256, 512
ROLE_TYPES = {(8, 2): (Q4, Q6, Q3), (64, 8): (Q2, Q8, Q5)}  # (gate, up, down): a different type per role
_mods = {}


def module(ops, E, dt):  # noqa: F811
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts
    if (E, dt) not in _mods:
        ex = PackedExperts(E, H, I, dt)
        K = 2 if E == 8 else 8
        for role, t in zip(M.ROLES, ROLE_TYPES[(E, K)]):
            R, Cr = ex.role_shape(role)
            ex.set_level(role, M.stacked(ops, t, E, R, Cr), t)
        _mods[(E, dt)] = ex
    return _mods[(E, dt)]


def hidden(T, dt):
    return torch.randn(T, H, generator=torch.Generator().manual_seed(10 * T)).to(dt).cuda()


def within(out, out64, B):
    err = (out.double() - out64).abs()
    return bool((err <= B).all()), float((err / B).max())


MODULE = [(E, K, dt) for E, K in ROLE_TYPES for dt in (F16, BF16)]
MODULE_IDS = [f"E{E}-K{K}-{str(dt)[6:]}" for E, K, dt in MODULE]


@pytest.mark.parametrize("E,K,dt", MODULE, ids=MODULE_IDS)
@pytest.mark.parametrize("T", [1, 8])
def test_module_decode_path(ops, E, K, dt, T):  # noqa: F811
    """Bit for bit the per-pair composition of ops.gemv_packed calls; it and the loop path within B of fp64."""
    ex = module(ops, E, dt)
    x = hidden(T, dt)
    idx, w = M.routing(T, E, K, seed=T + E)
    w = w.to(dt)
    assert ex.takes_decode_path(T, K)
    with torch.no_grad():
        got = ex(x, idx, w)
        want = M.composed_decode(ex, x, idx, w)
    assert got.shape == (T, H) and got.dtype == dt and bool(torch.isfinite(got).all()) and float(got.float().abs().max()) > 0
    assert torch.equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
    out64, B = M.fp64_and_bound(ex, x, idx, w)
    ok, worst = within(got, out64, B)
    ex.grouped_max_pairs = 0  # the loop path of the same module on the same inputs
    try:
        assert not ex.takes_decode_path(T, K) and not ex.takes_prefill_path(T, K)
        with torch.no_grad():
            loop = ex(x, idx, w)
    finally:
        del ex.grouped_max_pairs
    ok_loop, worst_loop = within(loop, out64, B)
    print(f"E={E} K={K} T={T} {dt}: decode err / B = {worst:.3f}, loop err / B = {worst_loop:.3f}")
    assert ok and ok_loop


@pytest.mark.parametrize("E,K,dt", MODULE, ids=MODULE_IDS)
@pytest.mark.parametrize("T", [33, 40])
def test_module_grouped_prefill(ops, E, K, dt, T):  # noqa: F811
    """prefill = "grouped": bit for bit the per-expert composition of ops.linear_packed calls, the same bits in three chunks;
    it and the loop path within B of fp64."""
    ex = module(ops, E, dt)
    x = hidden(T, dt)
    idx, w = M.routing(T, E, K, seed=T + E)
    w = w.to(dt)
    out64, B = M.fp64_and_bound(ex, x, idx, w)
    assert not ex.takes_prefill_path(T, K)
    with torch.no_grad():
        loop = ex(x, idx, w)
    ex.prefill = "grouped"
    try:
        assert ex.takes_prefill_path(T, K) and not ex.takes_decode_path(T, K)
        with torch.no_grad():
            got = ex(x, idx, w)
            want = M.composed_prefill(ex, x, idx, w)
        ex.prefill_max_pairs = 16 * K  # chunks of 16 tokens: 16, 16 and the rest
        assert len(range(0, T, 16)) == 3
        with torch.no_grad():
            parts = ex(x, idx, w)
    finally:
        del ex.prefill
        if "prefill_max_pairs" in vars(ex):
            del ex.prefill_max_pairs
    assert got.shape == (T, H) and got.dtype == dt and bool(torch.isfinite(got).all()) and float(got.float().abs().max()) > 0
    assert torch.equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
    assert torch.equal(bits(parts), bits(got)), "three chunks differ from one"
    (ok, worst), (ok_loop, worst_loop) = within(got, out64, B), within(loop, out64, B)
    print(f"E={E} K={K} T={T} {dt}: grouped prefill err / B = {worst:.3f}, loop err / B = {worst_loop:.3f}")
    assert ok and ok_loop


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_module_masked_pair_contributes_nothing(ops, dt):  # noqa: F811
    """E = 8: one pair of top_k_index is E (transformers' masked pair) and its weight is NaN.  The decode path (T = 8) and the
    grouped prefill (T = 33) are bit for bit their compositions over the other pairs, so the NaN was never multiplied in."""
    E, K = 8, 2
    ex = module(ops, E, dt)
    for T, composed in ((8, M.composed_decode), (33, M.composed_prefill)):
        x = hidden(T, dt)
        idx, w = M.routing(T, E, K, seed=T)
        w = w.to(dt)
        idx[1, 1] = E
        w[1, 1] = float("nan")
        ex.prefill = "grouped"
        try:
            assert ex.takes_decode_path(T, K) == (T == 8) and ex.takes_prefill_path(T, K) == (T == 33)
            with torch.no_grad():
                got = ex(x, idx, w)
                want = composed(ex, x, idx, w)
        finally:
            del ex.prefill
        assert bool(torch.isfinite(got).all()) and float(got[1].float().abs().max()) > 0
        assert torch.equal(bits(got), bits(want)), (T, int((bits(got) != bits(want)).sum()))
        out64, B = M.fp64_and_bound(ex, x, idx, w)
        assert within(got, out64, B)[0], T
