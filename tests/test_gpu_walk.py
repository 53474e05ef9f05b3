"""-m gpu: every kind of column walk (plain, stacked, slice, bands, act_order, uniform grids) through every schedule of
the walk, at the smallest shape that reaches them all.  R = 128, C = 2304, block 128 under la=4, far_async_min_sb=2 is 4.5
super-blocks of 512 columns on the helper-stream schedule: super-block 0 issues all three far launches ([512, 1024) on
the caller's stream, [1024, 1536) and [1536, 2304) on the helper), the later ones end short; the pair path and the
near256 kernel both run.  far_wgs=24 narrows the helper's persistent GEMM, far_sync=1 keeps the far updates on the
caller's stream, no_lookahead=1 updates after every block: all four must agree bit for bit, and the K-quant kinds must
equal the CPU oracle."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

Q4, Q6 = 12, 14
R, C, BLOCK = 128, 2304, 128
BASE = dict(la=4, far_async_min_sb=2)
SCHEDULES = [dict(), dict(far_wgs=24), dict(far_sync=1), dict(no_lookahead=1)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from gptq_gguf_toolkit_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _problem(oracle, rows, cols):
    """(W, U) as test_gptq_step_vs_oracle builds them"""
    rng = np.random.default_rng(rows + cols)
    W0 = (rng.standard_normal((rows, cols)) * 0.02).astype(np.float16).astype(np.float32)
    X = (rng.standard_normal((2 * cols, cols)) * np.exp(rng.standard_normal(cols) * 0.5)).astype(np.float32)
    H = oracle.h_accumulate(np.zeros((cols, cols), np.float32), X, 0.0, 2.0 / 4)
    U, _, W1, bad = oracle.h_prepare(H, W0, 0.01)
    assert not bad
    return W1, U


@pytest.fixture(scope="module")
def problem(oracle):
    """The shared (W, U) and, computed once per (rows, type), the oracle's step on those rows."""
    W1, U = _problem(oracle, R, C)
    refs = {}

    def ref(r0, r1, t):
        if (r0, r1, t) not in refs:
            refs[r0, r1, t] = oracle.gptq_step(W1[r0:r1], U, t, block_size=BLOCK)
        return refs[r0, r1, t]
    return W1, dev(U), ref


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _under_every_schedule(ops, run):
    """run() -> tuple of tensors, once per schedule; all four bit-identical.  -> the first one's."""
    outs = []
    with ops.options(**BASE):
        assert ops.uses_helper_stream(R, C, BLOCK)
    for extra in SCHEDULES:
        with ops.options(**BASE, **extra):
            torch.cuda.synchronize()  # the helper stream is idle: this call gets the lease
            outs.append(run())
            torch.cuda.synchronize()
    for extra, o in zip(SCHEDULES[1:], outs[1:]):
        assert len(o) == len(outs[0])
        for k, (a, b) in enumerate(zip(outs[0], o)):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bytes(a), _bytes(b)), f"{extra}: output {k}"
    return outs[0]


def _equals_oracle(got_W, got, want, tag):
    q, d, s, dmin, m = got
    Wd, oq, od, os_, odm, om = want
    u16 = lambda t: t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)  # noqa: E731
    assert np.array_equal(q.cpu().numpy(), oq), f"{tag}: {(q.cpu().numpy() != oq).mean():.4%} ints differ"
    assert np.array_equal(u16(d), od) and np.array_equal(u16(dmin), odm), tag
    assert np.array_equal(s.cpu().numpy(), os_) and np.array_equal(m.cpu().numpy(), om), tag
    assert np.array_equal(got_W.cpu().numpy(), Wd), tag


def test_plain(ops, problem):
    W1, U, ref = problem

    def run():
        W = dev(W1)
        return (W,) + tuple(ops.gptq_quantize(W, U, Q4, block_size=BLOCK))
    out = _under_every_schedule(ops, run)
    _equals_oracle(out[0], out[1:], ref(0, R, Q4), "plain")


def test_stacked(ops, problem):
    W1, U, ref = problem

    def run():
        W = dev(W1)
        return (W,) + tuple(ops.gptq_quantize(W, U, Q4, block_size=BLOCK, row_ends=[64, 128]))
    out = _under_every_schedule(ops, run)
    for r0, r1 in ((0, 64), (64, 128)):
        _equals_oracle(out[0][r0:r1], [t[r0:r1] for t in out[1:]], ref(r0, r1, Q4), f"stacked rows {r0}:{r1}")


def test_slice(ops, problem):
    W1, U, ref = problem

    def run():
        W = dev(W1)
        n = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        return (W,) + tuple(ops.gptq_quantize(W, U, Q4, block_size=BLOCK, panel_researches=n)) + (n,)
    out = _under_every_schedule(ops, run)
    assert int(out[6].item()) >= 0  # the count was written (and is the same under every schedule)
    _equals_oracle(out[0], out[1:6], ref(0, R, Q4), "slice")


def test_bands(ops, problem):
    W1, U, ref = problem

    def run():
        W = dev(W1)
        bands = ops.gptq_quantize_bands(W, U, [(64, Q4), (128, Q6)], block_size=BLOCK)
        return (W,) + tuple(t for band in bands for t in band)
    out = _under_every_schedule(ops, run)
    for k, (r0, r1, t) in enumerate(((0, 64, Q4), (64, 128, Q6))):
        _equals_oracle(out[0][r0:r1], out[1 + 5 * k:6 + 5 * k], ref(r0, r1, t), f"band rows {r0}:{r1} type {t}")


def _perm_inputs(ops, W1, cols, seed):
    """static scales of the original column groups (the fp32 RTN search) and a fixed random permutation; U is taken as it
    is -- the walk is the same arithmetic for any upper-triangular U"""
    perm = np.random.default_rng(seed).permutation(cols).astype(np.int32)
    _, d, s, dmin, m = ops.rtn_quantize(dev(W1), Q4)
    return perm, torch.from_numpy(perm).cuda(), (d, s, dmin, m)


def test_perm(ops, problem):
    W1, U, _ = problem
    perm, permd, scales = _perm_inputs(ops, W1, C, 7)

    def run():
        W = dev(W1[:, perm])
        return W, ops.gptq_quantize_perm(W, U, Q4, permd, *scales, block_size=BLOCK)
    _under_every_schedule(ops, run)


def test_obq(ops, problem):
    W1, U, _ = problem

    def run():
        W = dev(W1)
        return (W,) + tuple(ops.obq_quantize(W, U, 4, group_size=128, block_size=BLOCK))
    _under_every_schedule(ops, run)


@pytest.mark.parametrize("kind", ["perm", "obq"])
def test_a_straddling_block_stays_inside_its_workspace(ops, oracle, kind):
    """block_size 96 at C = 512: the block of columns 192 .. 287 lives in the block scratch.  With a workspace of exactly
    workspace_bytes, nothing behind it is written by the act_order walk and the uniform-grid walk (the K-quant and band
    walks: test_gpu_levels.py), and the results are those of a call with a workspace of its own."""
    from gptq_gguf_toolkit_amd import _cabi
    rows, cols, block = 128, 512, 96
    W1, U = _problem(oracle, rows, cols)
    Ud = dev(U)
    need = ops.workspace_bytes(_cabi.WS_GPTQ_QUANTIZE, rows, cols, 0, block)
    assert need >= 2 * rows * block * 4  # the error buffer and the block scratch
    if kind == "perm":
        perm, permd, scales = _perm_inputs(ops, W1, cols, 11)
        W1 = W1[:, perm]

    def run(ws):
        W = dev(W1)
        if kind == "perm":
            return W, ops.gptq_quantize_perm(W, Ud, Q4, permd, *scales, block_size=block, ws=ws)
        return (W,) + tuple(ops.obq_quantize(W, Ud, 4, group_size=128, block_size=block, ws=ws))
    guard = 1 << 20
    buf = torch.full((need + guard,), 0xAB, dtype=torch.uint8, device="cuda")
    got = run(buf[:need])
    torch.cuda.synchronize()
    assert bool((buf[need:] == 0xAB).all()), "bytes behind the workspace were written"
    for a, b in zip(got, run(None)):
        assert torch.equal(_bytes(a), _bytes(b))
