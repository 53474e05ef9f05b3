"""-m gpu: every regime of the Cholesky chain (gq_h_prepare, csrc/gq_cholesky.hip walking csrc/gq_chol_plan.hpp), pinned
bit for bit against the chain as it was before the plan existed.

A case is (C, library options, obq_order).  The Hessian is test_gpu_widest_chain's _image_hessian (correlated, one dead row,
one row whose off-diagonal entries are subnormal), W is 64 x C from a seeded generator.  Everything the call produces --
U, the flag, col_flags, and W and H as the call leaves them in place -- must have the CRC32 recorded from the recursion
that decided each node's regime while it launched (tests/golden/chol_regimes_crc.json; `python
tests/test_gpu_chol_regimes.py --record FILE` writes the table).  The sizes are the smallest that reach each regime under
the default thresholds: 128 is one leaf, 384 an uneven split, 1280 paired fp32 nodes only, 2048 a split-bf16 node over
fp32 ones, 4096 image GEMMs over split-bf16 over paired fp32 (tests/test_chol_plan_cpu.py asserts exactly this of the
plan).  chol_3p_min=128 at four widths stays with test_gpu_widest_chain.py."""
import json
import os
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GOLDEN  # noqa: E402  (puts the repo root on sys.path)
from test_gpu_widest_chain import _image_hessian  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

R = 64
CRC_FILE = os.path.join(GOLDEN, "chol_regimes_crc.json")
# name -> (C, library options, obq_order)
CASES = {
    "C128": (128, {}, False),
    "C384": (384, {}, False),
    "C384-diag_ref": (384, dict(diag_ref=1), False),
    "C384-obq_order": (384, {}, True),
    "C1280": (1280, {}, False),
    "C1280-no_pair": (1280, dict(chol_no_pair=1), False),
    "C2048": (2048, {}, False),
    "C2048-fp32": (2048, dict(chol_fp32=1, chol_3p_min=0), False),
    "C4096": (4096, {}, False),
    "C4096-planes3": (4096, dict(chol_planes=3), False),
    "C4096-3p_min0": (4096, dict(chol_3p_min=0), False),
    "C4096-no_equil": (4096, dict(chol_no_equil=1), False),
    "C4096-poison": (4096, dict(chol_poison=1), False),
}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from gptq_gguf_toolkit_amd import ops as _ops
    return _ops


_inputs = {}  # C -> (H, W), built once and never written: every case works on clones


def _crcs(ops, name):
    C, opts, obq_order = CASES[name]
    if C not in _inputs:
        W = torch.randn(R, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(C))
        _inputs[C] = (_image_hessian(ops, C), W)
    H, W = (t.clone() for t in _inputs[C])
    with ops.options(**opts):
        U, flag, col_flags = ops.h_prepare(H, W, 0.01, want_flags=True, obq_order=obq_order)
        torch.cuda.synchronize()
    assert int(flag.item()) == 0
    assert bool(torch.isfinite(U).all())
    out = dict(U=U, flag=flag, col_flags=col_flags, W=W, H=H)
    return {k: zlib.crc32(v.cpu().numpy().tobytes()) for k, v in out.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_outputs_are_the_recorded_ones(ops, name):
    with open(CRC_FILE) as f:
        want = json.load(f)
    assert _crcs(ops, name) == want[name]


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: test_gpu_chol_regimes.py --record FILE"
    from gptq_gguf_toolkit_amd import ops as _ops
    table = {name: _crcs(_ops, name) for name in CASES}
    with open(sys.argv[2], "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print(table)
