"""-m gpu: the two pieces of the widest chain's serial path that changed shape, pinned bit for bit.

Helper form of the column walk (gq_gptq.hip, FarPipeline): R = 128, C = 1024, block 128 under la=2, far_async_min_sb=2
is four super-blocks of 256 columns on the helper-stream schedule, so every event of the pipeline fires: `ready` behind
F_s[s+1], ev_small_prev, both halves of ev_bulk and the final wait.  The ragged case -- a last column group shorter than
la * 128, where g1 / g2 of the last far updates are clamped to C -- was specified as C = 1152, which every walk refuses
(C % 256 != 0), and no C that it accepts is ragged under la=2; the smallest ragged shape is C = 1280 under la=4 (2.5
super-blocks of 512: F_0[2] is cut to [1024, 1280), F_0[3..] is empty, F_1[2] is cut and is the walk's last far
update).  W and all five outputs must be the same bytes with and without the helper stream, and equal to the CPU oracle
on the same U.

Imaging (gq_gemm3p.hpp, launch_split<2>): gq_h_prepare under chol_3p_min=128 on correlated Hessians (corr_hessian.py)
with one zero row and one row whose largest off-diagonal entry is subnormal.  C = 512 and 1280 are the cases the change
was specified with (1280 = halves of 640, not a multiple of 256: it stays off the image path and must stay what it was);
C = 1024 and 1536 add image nodes with K = 512 / 256 and K = 768 (24 chunks: the 16-chunk stride of the one-pass kernel
ends ragged) and `tri` panels beyond the first.  U must have the CRC32 recorded from the two-pass form
(tests/golden/widest_chain_u_crc.json; `python tests/test_gpu_widest_chain.py --record FILE` writes the table)."""
import json
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GOLDEN  # noqa: E402  (puts the repo root on sys.path)
from corr_hessian import correlated_x  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

Q3, Q4 = 11, 12
R, BLOCK = 128, 128
WALK_SHAPES = [(1024, 2), (1280, 4)]  # (C, la), both under far_async_min_sb=2
IMAGE_C = (512, 1280, 1024, 1536)
CRC_FILE = os.path.join(GOLDEN, "widest_chain_u_crc.json")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from gptq_gguf_toolkit_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bytes(t):
    return t.contiguous().view(torch.uint8)


# ----------------------------------------------------------------- the helper form of the walk
@pytest.fixture(scope="module", params=WALK_SHAPES, ids=lambda p: f"C{p[0]}-la{p[1]}")
def walk_problem(request, oracle):
    """(C, la, W, U) as test_gptq_step_vs_oracle builds them, shared by both types"""
    C, la = request.param
    rng = np.random.default_rng(R + C)
    W0 = (rng.standard_normal((R, C)) * 0.02).astype(np.float16).astype(np.float32)
    X = (rng.standard_normal((2 * C, C)) * np.exp(rng.standard_normal(C) * 0.5)).astype(np.float32)
    H = oracle.h_accumulate(np.zeros((C, C), np.float32), X, 0.0, 2.0 / 4)
    U, _, W1, bad = oracle.h_prepare(H, W0, 0.01)
    assert not bad
    return C, la, W1, U


@pytest.mark.parametrize("q_type", [Q4, Q3])
def test_helper_form_is_the_one_stream_walk_and_the_oracle(ops, oracle, walk_problem, q_type):
    C, la, W1, U = walk_problem
    Ud = dev(U)
    outs = {}
    was = ops.far_helper_enable(True)
    try:
        with ops.options(la=la, far_async_min_sb=2):
            assert ops.uses_helper_stream(R, C, BLOCK)
            for helper in (True, False):
                ops.far_helper_enable(helper)
                torch.cuda.synchronize()  # the helper stream is idle: this call gets the lease
                W = dev(W1)
                outs[helper] = (W,) + tuple(ops.gptq_quantize(W, Ud, q_type, block_size=BLOCK))
                torch.cuda.synchronize()
    finally:
        ops.far_helper_enable(was)
    assert len(outs[True]) == len(outs[False]) == 6
    for k, (a, b) in enumerate(zip(outs[True], outs[False])):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bytes(a), _bytes(b)), f"output {k}"
    Wd, oq, od, os_, odm, om = oracle.gptq_step(W1, U, q_type, block_size=BLOCK)
    W, q, d, s, dmin, m = outs[True]
    u16 = lambda t: t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)  # noqa: E731
    assert np.array_equal(q.cpu().numpy(), oq), f"{(q.cpu().numpy() != oq).mean():.4%} ints differ"
    assert np.array_equal(u16(d), od) and np.array_equal(u16(dmin), odm)
    assert np.array_equal(s.cpu().numpy(), os_) and np.array_equal(m.cpu().numpy(), om)
    assert np.array_equal(W.cpu().numpy(), Wd)


# ----------------------------------------------------------------- imaging
def _image_hessian(ops, C):
    """A correlated Hessian whose lower-left block has a zero row (a dead channel: row and column 3C/4 + 5 are zero)
    and a row whose largest entry is subnormal (row and column 3C/4 + 9 are +-1e-42 off the diagonal)."""
    X = correlated_x(2 * C, C, rank=C // 16, eps=0.3, seed=C, massive=0)
    H = torch.zeros(C, C, device="cuda")
    ops.h_accumulate(H, X, 0.0, 2.0 / 8)
    i, j = 3 * C // 4 + 5, 3 * C // 4 + 9
    H[i, :] = 0.0
    H[:, i] = 0.0
    djj = H[j, j].clone()
    tiny = torch.full((C,), 1e-42, device="cuda")
    tiny[1::2] = -1e-42
    H[j, :] = tiny
    H[:, j] = tiny
    H[j, j] = djj
    assert 0.0 < float(H[j, :C // 2].abs().max()) < 1.1754944e-38  # still subnormal on the device
    return H


def _u_crc(ops, C):
    H = _image_hessian(ops, C)
    W = torch.randn(64, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(C))
    with ops.options(chol_3p_min=128):
        U, flag = ops.h_prepare(H, W, 0.01)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    assert bool(torch.isfinite(U).all())
    return zlib.crc32(U.cpu().numpy().tobytes())


@pytest.mark.parametrize("C", IMAGE_C)
def test_u_is_the_recorded_two_pass_u(ops, C):
    with open(CRC_FILE) as f:
        want = json.load(f)
    assert _u_crc(ops, C) == want[str(C)]


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: test_gpu_widest_chain.py --record FILE"
    from gptq_gguf_toolkit_amd import ops as _ops
    table = {str(C): _u_crc(_ops, C) for C in IMAGE_C}
    with open(sys.argv[2], "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print(table)
