"""-m gpu: the column-loop segment kernel (gq_gptq.hip, gptq_segment_kernel) after its tile loop was rolled and its group
parameters moved to LDS, pinned bit for bit in all four instantiations.

Every case runs one walk at the smallest shape that reaches the path it names, and its outputs -- the written-back W
and what the walk returns -- must equal (a) the CPU oracle on the same (W, U) and (b) the CRC32 recorded from the
library as it was BEFORE the kernel changed (tests/golden/segment_codeobj_crc.json;
`python tests/test_gpu_segment_codeobj.py --record FILE` writes the table, with GQ_SO_PATH naming the library to record).

Shapes: R = 64 (one workgroup), 192 (three), 100 (ragged: the `live` mask); C = 256 (one pair group: the epilogue and the
partner block in one launch), 512, and 1280 under la = 4 (a short last super-block); block 192 cuts every block into a
128- and a 64-column segment through the block scratch (no pair launch).  Kinds: the four K-quants (16- and 32-column
groups, signed and unsigned), act_order, the uniform grid at 3 and 4 bits, two bands of different types, a stacked
call."""
import json
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GOLDEN  # noqa: E402  (puts the repo root on sys.path)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

Q2, Q3, Q4, Q6 = 10, 11, 12, 14
CRC_FILE = os.path.join(GOLDEN, "segment_codeobj_crc.json")

# id -> (kind, R, C, block, walk options, kind's argument)
CASES = {
    "Q4_K-R64-C256": ("kquant", 64, 256, 128, {}, Q4),
    "Q2_K-R192-C512": ("kquant", 192, 512, 128, {}, Q2),
    "Q3_K-R100-C512": ("kquant", 100, 512, 128, {}, Q3),
    "Q6_K-R100-C1280-la4": ("kquant", 100, 1280, 128, dict(la=4), Q6),
    "Q4_K-R100-C512-b192": ("kquant", 100, 512, 192, {}, Q4),
    "Q6_K-R64-C512-b192": ("kquant", 64, 512, 192, {}, Q6),
    "perm-Q4_K-R100-C512": ("perm", 100, 512, 128, {}, Q4),
    "perm-Q6_K-R64-C256": ("perm", 64, 256, 128, {}, Q6),
    "uni3-R64-C512": ("uniform", 64, 512, 128, {}, 3),
    "uni4-R100-C256": ("uniform", 100, 256, 128, {}, 4),
    "bands-Q4_K-Q6_K-R128-C512": ("bands", 128, 512, 128, {}, [(64, Q4), (128, Q6)]),
    "bands-Q2_K-Q3_K-R192-C1280-la4": ("bands", 192, 1280, 128, dict(la=4), [(128, Q2), (192, Q3)]),
    "stacked-Q4_K-R192-C512": ("stacked", 192, 512, 128, {}, [64, 128, 192]),
}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(t):
    """a tensor's bytes as a numpy array (fp16 scales as their bit patterns)"""
    return t.detach().contiguous().cpu().view(torch.uint8).numpy()


_problems = {}


def _problem(O, R, C):
    """(W, U) as test_gptq_step_vs_oracle builds them, once per shape"""
    if (R, C) not in _problems:
        rng = np.random.default_rng(R + C)
        W0 = (rng.standard_normal((R, C)) * 0.02).astype(np.float16).astype(np.float32)
        X = (rng.standard_normal((2 * C, C)) * np.exp(rng.standard_normal(C) * 0.5)).astype(np.float32)
        H = O.h_accumulate(np.zeros((C, C), np.float32), X, 0.0, 2.0 / 4)
        U, _, W1, bad = O.h_prepare(H, W0, 0.01)
        assert not bad
        _problems[R, C] = (W1, U)
    return _problems[R, C]


def _perm_inputs(ops, W1, C, q_type):
    perm = np.random.default_rng(C + q_type).permutation(C).astype(np.int32)
    _, d, s, dmin, m = ops.rtn_quantize(dev(W1), q_type)  # static scales of the original groups
    return perm, (d, s, dmin, m)


def _run(ops, O, case):
    """-> (inputs the oracle needs, {output name: device tensor})"""
    kind, R, C, block, opts, arg = CASES[case]
    W1, U = _problem(O, R, C)
    Ud = dev(U)
    extra = None
    with ops.options(**opts):
        if kind == "kquant":
            W = dev(W1)
            outs = dict(zip("q d s dmin m".split(), ops.gptq_quantize(W, Ud, arg, block_size=block)))
        elif kind == "stacked":
            W = dev(W1)
            outs = dict(zip("q d s dmin m".split(), ops.gptq_quantize(W, Ud, Q4, block_size=block, row_ends=arg)))
        elif kind == "perm":
            perm, scales = _perm_inputs(ops, W1, C, arg)
            extra = (perm, scales)
            W = dev(W1[:, perm])
            outs = {"q": ops.gptq_quantize_perm(W, Ud, arg, dev(perm), *scales, block_size=block)}
        elif kind == "uniform":
            W = dev(W1)
            outs = dict(zip("q scale zero".split(), ops.obq_quantize(W, Ud, arg, group_size=128, block_size=block)))
        else:
            W = dev(W1)
            bands = ops.gptq_quantize_bands(W, Ud, arg, block_size=block)
            outs = {f"{n}{k}": t for k, band in enumerate(bands) for n, t in zip("q d s dmin m".split(), band)}
        torch.cuda.synchronize()
    outs["W"] = W
    return (W1, U, extra), outs


def _crcs(outs):
    return {n: zlib.crc32(_raw(t).tobytes()) for n, t in sorted(outs.items())}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from gptq_gguf_toolkit_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def results(ops, oracle):
    """every case is walked once; both tests read it"""
    done = {}

    def get(case):
        if case not in done:
            done[case] = _run(ops, oracle, case)
        return done[case]
    return get


def _same(got, want, tag):
    g, w = _raw(got).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert g.size == w.size and np.array_equal(g, w), tag


def _kquant_equal(outs, sfx, rows, want, tag):
    Wd, oq, od, os_, odm, om = want
    r0, r1 = rows
    _same(outs["W"][r0:r1], Wd, f"{tag}: W")
    for n, w in (("q", oq), ("d", od), ("s", os_), ("dmin", odm), ("m", om)):
        t = outs[n + sfx]
        _same(t if sfx else t[r0:r1], w, f"{tag}: {n}")


@pytest.mark.parametrize("case", list(CASES))
def test_equals_the_oracle(oracle, results, case):
    kind, R, C, block, _, arg = CASES[case]
    (W1, U, extra), outs = results(case)
    if kind == "kquant":
        _kquant_equal(outs, "", (0, R), oracle.gptq_step(W1, U, arg, block_size=block), case)
    elif kind == "stacked":
        for r0, r1 in zip([0] + arg[:-1], arg):
            _kquant_equal(outs, "", (r0, r1), oracle.gptq_step(W1[r0:r1], U, Q4, block_size=block), f"{case} rows {r0}:{r1}")
    elif kind == "bands":
        r0 = 0
        for k, (r1, t) in enumerate(arg):
            _kquant_equal(outs, str(k), (r0, r1), oracle.gptq_step(W1[r0:r1], U, t, block_size=block), f"{case} band {k}")
            r0 = r1
    elif kind == "perm":
        perm, (d, s, dmin, m) = extra
        npy = lambda t: t.cpu().numpy()  # noqa: E731
        Wd, oq = oracle.gptq_step_perm(W1[:, perm], U, arg, perm, _raw(d).view(np.uint16), npy(s), _raw(dmin).view(np.uint16),
                                       npy(m), block_size=block)
        _same(outs["W"], Wd, f"{case}: W")
        _same(outs["q"], oq, f"{case}: q")
    else:
        Wd, oq, sc, ze = oracle.obq_step(W1, U, arg, group_size=128, block_size=block)
        for n, w in (("W", Wd), ("q", oq), ("scale", sc), ("zero", ze)):
            _same(outs[n], w, f"{case}: {n}")


@pytest.mark.parametrize("case", list(CASES))
def test_equals_the_recorded_crc(results, case):
    with open(CRC_FILE) as f:
        want = json.load(f)
    assert _crcs(results(case)[1]) == want[case]


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: test_gpu_segment_codeobj.py --record FILE"
    from gptq_gguf_toolkit_amd import _cabi, ops as _ops
    from oracle import oracle as _O
    _O.build()
    table = {case: _crcs(_run(_ops, _O, case)[1]) for case in CASES}
    with open(sys.argv[2], "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print("recorded from", _cabi.SO_PATH)
    print(table)
