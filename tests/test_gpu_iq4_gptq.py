"""-m gpu: GPTQ's column walk on the IQ4_XS / IQ4_NL grid (gq_gptq_quantize_iq4, gq_pack_iq4; include/gptq_gguf_iq4_gptq.h)
against the loop restatement of its contract (tests/iq4_gptq_spec.py), bit for bit, and the two consequences of the contract
without the spec: with U = I the packed bytes are gq_quantize_iq4's, and the returned W is the decode of the packed bytes.

Shapes are the smallest that reach the path they name: R = 64 (one workgroup), 100 / 70 (ragged: the `live` mask), 192
(three workgroups); C = 256 (one pair group), 512, 768, and 1280 under la = 4 (a short last super-block); block 192 cuts every
block into a 128- and a 64-column segment through the block scratch, 64 and 256 leave the look-ahead path.  Problems are built
as tests/test_gpu_segment_codeobj.py builds them: U comes from the oracle's h_prepare."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT  # noqa: E402,F401  (puts the repo root on sys.path)

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))  # make_golden_shim: the tiny Llama of the level-build tests

import iq4_encode_spec as ES  # noqa: E402
import iq4_gptq_spec as S  # noqa: E402
from test_gpu_segment_codeobj import _problem, _raw, dev  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NL, XS = S.NL, S.XS
# id -> (type, R, C, block, walk options, with importance)
CASES = {
    "XS-R64-C256": (XS, 64, 256, 128, {}, False),
    "XS-R100-C512-imp": (XS, 100, 512, 128, {}, True),
    "NL-R70-C768": (NL, 70, 768, 128, {}, False),
    "XS-R100-C512-b192": (XS, 100, 512, 192, {}, False),
    "XS-R64-C512-b64": (XS, 64, 512, 64, {}, False),
    "XS-R64-C512-b256": (XS, 64, 512, 256, {}, False),
    "XS-R192-C1280-la4": (XS, 192, 1280, 128, dict(la=4), False),
    "NL-R64-C256-imp": (NL, 64, 256, 128, {}, True),
}
GUARD = 64  # guard elements on either side of every output


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from gptq_gguf_toolkit_amd import ops as _ops
    return _ops


def _walk(ops, W0, U, t, block=128, imp=None, **opts):
    """-> dict of device tensors W, qweight, d, ls, step"""
    W = dev(W0)
    with ops.options(**opts):
        q, d, ls, step = ops.gptq_quantize_iq4(W, dev(U), t, block_size=block, importance=None if imp is None else dev(imp))
        torch.cuda.synchronize()
    return dict(W=W, qweight=q, d=d, ls=ls, step=step)


def _same(got, want, tag):
    g, w = _raw(got).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert g.size == w.size and np.array_equal(g, w), tag


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_equals_the_spec(ops, oracle, case):
    t, R, C, block, opts, weighted = CASES[case]
    W1, U = _problem(oracle, R, C)
    imp = ES.random_importance(C, R) if weighted else None
    got = _walk(ops, W1, U, t, block, imp, **opts)
    want = S.walk(W1, U, t, block, imp)
    for n in ("qweight", "d", "step", "W") + (("ls",) if t == XS else ()):
        _same(got[n], want[n], f"{case}: {n}")
    assert got["ls"] is None or t == XS


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("t", [XS, NL])
@pytest.mark.parametrize("shape", [(70, 512), (64, 768)])
def test_with_the_identity_the_packed_bytes_are_the_encoders(ops, shape, t, weighted):
    R, C = shape
    W0 = ES.random_matrix(R, C, R + t)
    imp = ES.random_importance(C, C) if weighted else None
    out = _walk(ops, W0, np.eye(C, dtype=np.float32), t, 128, imp)
    packed = ops.pack_iq4(t, out["qweight"], out["d"], out["ls"])
    want = ops.quantize_iq4(dev(W0), t, None if imp is None else dev(imp))
    assert torch.equal(packed, want)


@pytest.mark.parametrize("t", [XS, NL])
def test_w_is_the_decode_of_the_packed_bytes(ops, oracle, t):
    R, C = 100, 512
    W1, U = _problem(oracle, R, C)
    out = _walk(ops, W1, U, t)
    src = torch.from_numpy(np.random.default_rng(3).permutation(R).astype(np.int32)).cuda()
    for row_src in (None, src):
        dec = ops.dequantize_blocks(t, ops.pack_iq4(t, out["qweight"], out["d"], out["ls"], row_src))
        want = out["W"] if row_src is None else out["W"][row_src.long()]
        assert not torch.isnan(dec).any() and bool((dec == want).all())  # == on values: the sign of a zero is not compared
    assert not torch.equal(out["W"], dev(W1))


@pytest.mark.parametrize("t", [XS, NL])
def test_degenerate_inputs(ops, oracle, t):
    R, C = 64, 512
    W1, U = _problem(oracle, R, C)
    W1 = W1.copy()
    U = np.eye(C, dtype=np.float32)  # (zero columns stay zero only without error feedback into them)
    W1[:, 256:] = 0                  # an all-zero super-block in every row
    W1[:, 32:64] = 0                 # an all-zero block inside a live super-block
    imp = ES.random_importance(C, 9)
    imp[96:128] = 0                  # importance all zero over one block
    got = _walk(ops, W1, U, t, 128, imp)
    want = S.walk(W1, U, t, 128, imp)
    for n in ("qweight", "d", "step", "W") + (("ls",) if t == XS else ()):
        _same(got[n], want[n], n)
    q, W = got["qweight"].cpu().numpy(), got["W"].cpu().numpy()
    assert (q[:, 256:] == 8).all() and (q[:, 32:64] == 8).all() and not W[:, 256:].any() and not W[:, 32:64].any()
    assert not np.isnan(W).any()


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(*shape)


@pytest.mark.parametrize("t", [XS, NL])
def test_guard_bytes_around_every_output_are_untouched(ops, oracle, t):
    from gptq_gguf_toolkit_amd import _cabi
    R, C = 100, 512  # ragged rows: the last workgroup is partly dead
    W1, U = _problem(oracle, R, C)
    L, p = _cabi.lib(), lambda x: x.data_ptr()
    Wb, W = _guarded((R, C), torch.float32, 7.0)
    W.copy_(dev(W1))
    qb, q = _guarded((R, C), torch.uint8, 0xA5)
    db, d = _guarded((R, C // 256 if t == XS else C // 32), torch.float16, 7.0)
    lb, ls = _guarded((R, C // 32), torch.uint8, 0xA5)
    sb, step = _guarded((R, C // 32), torch.float32, 7.0)
    ib, istep = _guarded((R, C // 32), torch.float32, 7.0)
    need = ops.workspace_bytes(_cabi.WS_GPTQ_QUANTIZE, R, C, 0, 128)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    Ud = dev(U)
    _cabi.check(L.gq_gptq_quantize_iq4(p(W), p(Ud), R, C, t, 128, None, p(q), p(d), p(ls) if t == XS else None, p(step), p(istep),
                                       p(ws), need, None), "gq_gptq_quantize_iq4")
    nbytes = R * (C // 256 * 136 if t == XS else C // 32 * 18)
    ob = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    _cabi.check(L.gq_pack_iq4(t, R, C, p(q), p(d), p(ls) if t == XS else None, None, p(ob) + GUARD, None), "gq_pack_iq4")
    torch.cuda.synchronize()
    for buf, fill in ((Wb, 7.0), (qb, 0xA5), (db, 7.0), (sb, 7.0), (ib, 7.0), (ob, 0xA5), (lb, 0xA5)):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())
    if t == NL:
        assert bool((lb == 0xA5).all())  # IQ4_NL never touches ls
    assert torch.equal(ob[GUARD:-GUARD].view(R, -1), ops.pack_iq4(t, q, d, ls if t == XS else None))
    assert bool((ops.dequantize_blocks(t, ob[GUARD:-GUARD].view(R, -1).clone()) == W).all())


def test_refusals_through_ops(ops):
    from gptq_gguf_toolkit_amd import _cabi
    W, U = torch.zeros(64, 256, device="cuda"), torch.eye(256, device="cuda")
    with pytest.raises(_cabi.GQError, match="neither IQ4_NL"):
        ops.gptq_quantize_iq4(W, U, 12)
    with pytest.raises(_cabi.GQError, match="C=288|C %"):
        ops.gptq_quantize_iq4(torch.zeros(64, 288, device="cuda"), torch.eye(288, device="cuda"), XS)
    with pytest.raises(_cabi.GQError, match="importance"):
        ops.gptq_quantize_iq4(W, U, XS, importance=torch.zeros(255, device="cuda"))
    with pytest.raises(_cabi.GQError, match="workspace"):
        L = _cabi.lib()
        b = torch.zeros(64 * 256, dtype=torch.float32, device="cuda")
        _cabi.check(L.gq_gptq_quantize_iq4(W.data_ptr(), U.data_ptr(), 64, 256, XS, 128, None, b.data_ptr(), b.data_ptr(),
                                           b.data_ptr(), b.data_ptr(), b.data_ptr(), b.data_ptr(), 16, None), "walk")
    with pytest.raises(_cabi.GQError, match="importance"):  # misaligned importance at the C ABI
        _cabi.check(L.gq_gptq_quantize_iq4(W.data_ptr(), U.data_ptr(), 64, 256, XS, 128, b.data_ptr() + 4, b.data_ptr(),
                                           b.data_ptr(), b.data_ptr(), b.data_ptr(), b.data_ptr(), b.data_ptr(), 1 << 30, None), "walk")
    torch.cuda.synchronize()
    assert not W.any()  # nothing was launched


def test_quality_on_the_device(ops):
    """The two correlated problems of tests/test_iq4_gptq_cpu.py with U from ops.h_prepare: the relative error
    sum(dW H o dW) / sum(W H o W) of the walk's W, on the host in fp64, below half of gq_quantize_iq4's with the same importance."""
    for W0, H, diag in S.quality_problems():
        C = W0.shape[1]
        Hu = (H - 0.01 * np.mean(diag.astype(np.float64)) * np.eye(C)).astype(np.float32)  # undamped: h_prepare damps by 1 %
        U, bad = ops.h_prepare(dev(Hu), dev(W0), 0.01)
        assert not int(bad.item())
        W = dev(W0)
        ops.gptq_quantize_iq4(W, U, XS, importance=dev(diag))
        rtn = ops.dequantize_blocks(XS, ops.quantize_iq4(dev(W0), XS, dev(diag)))
        e_gptq = S.relative_error(W0, W.cpu().numpy(), H)
        e_rtn = S.relative_error(W0, rtn.cpu().numpy(), H)
        print(f"[{W0.shape[0]} x {C}] RTN {e_rtn:.3e}  GPTQ {e_gptq:.3e}  ratio {e_gptq / e_rtn:.3f}")
        assert e_gptq < 0.5 * e_rtn


# ------------------------------------------------------------------------------------------------ the level build
STEM = {XS: "4.25-IQ4_XS", NL: "4.56-IQ4_NL"}


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """Two level builds of the tiny Llama as tests/test_gpu_iq4_encode.py sets them up (levels Q2_K and Q4_K, both IQ4 types,
    diag(H) as importance): db_rtn with level_db_iq4_method="rtn", db_gptq with "gptq"."""
    from make_golden_shim import tiny_calib, tiny_llama
    from test_gpu_iq4_encode import _drive
    root = tmp_path_factory.mktemp("iq4_gptq_levels")
    keep = os.environ.get("GQ_SAVE_SLOT_MB")
    os.environ["GQ_SAVE_SLOT_MB"] = "8"  # the tiny model's files: no large staging slots to pin per run
    try:
        for method in ("rtn", "gptq"):
            _drive(root, method, root / "model", level_db_iq4=("IQ4_XS", "IQ4_NL"), level_db_iq4_method=method)
    finally:
        if keep is None:
            os.environ.pop("GQ_SAVE_SLOT_MB", None)
        else:
            os.environ["GQ_SAVE_SLOT_MB"] = keep
    model = tiny_llama(dtype=torch.float16).cuda()
    names = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and "layers" in n]
    assert len(names) == 14
    return {"root": root, "rtn": root / "db_rtn", "gptq": root / "db_gptq", "model": model, "names": names, "calib": tiny_calib()}


def _files(db, suffix):
    return sorted(os.path.relpath(os.path.join(d, f), db) for d, _, fs in os.walk(db) for f in fs if f.endswith(suffix))


def test_level_build_with_the_walk_changes_the_iq4_levels_of_the_linears_only(builds):
    from gptq_gguf_toolkit_amd import level_db as ldb
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import map_tensor_name
    rtn, gptq, names = builds["rtn"], builds["gptq"], builds["names"]
    assert _files(gptq, ".pth") == _files(rtn, ".pth") and _files(gptq, ".json") == _files(rtn, ".json")
    linear_iq4 = {f"{map_tensor_name(n + '.weight')}/{STEM[t]}.pth" for n in names for t in (XS, NL)}
    assert linear_iq4 <= set(_files(gptq, ".pth"))  # both files of every packed Linear
    import json
    ma, mb = json.load(open(gptq / "manifest.json")), json.load(open(rtn / "manifest.json"))
    assert ma["layers"] == mb["layers"] and list(ma["layers"]) == list(mb["layers"]) and ma["metadata"] == mb["metadata"]
    for n in names:  # registered before the K-quant levels: the tensor's database record stays its last K-quant level
        assert list(ma["layers"][map_tensor_name(n + ".weight")]["bitwidths"]) == ["4.25", "4.56", "2.5625", "4.5"]
    for f in _files(gptq, ".pth") + _files(gptq, ".json"):
        if f == "manifest.json":  # (holds the build's time stamp: its layers and key/value data were compared above)
            continue
        same = (gptq / f).read_bytes() == (rtn / f).read_bytes()
        # every K-quant file, every record, gguf_layer_database.json, and the IQ4 files of embed / lm_head: byte for byte
        assert same != (f in linear_iq4), f
    assert (gptq / "gguf_layer_database.json").read_bytes() == (rtn / "gguf_layer_database.json").read_bytes()
    for n in names:
        shape = tuple(builds["model"].get_submodule(n).weight.shape)
        for key in (4.25, 4.56):
            w = ldb.load_level(ldb.find_level_file(ldb.layer_dir(str(gptq), n), key), "cuda", str(gptq))
            assert tuple(w.shape) == shape and bool(torch.isfinite(w).all()), (n, key)


def test_the_estimator_prefers_the_walks_level(builds):
    """The estimator's summed layer error of every level, under both methods; the IQ4_XS level of the walk is strictly below
    the round-to-nearest one."""
    from make_golden_shim import tiny_llama
    from gptq_gguf_toolkit_amd.error_estimator import ErrorEstimator
    from test_gpu_iq4_encode import LINEARS
    data = [([], {"input_ids": ids}) for ids in builds["calib"]]
    total = {}
    for method in ("rtn", "gptq"):
        est = ErrorEstimator(tiny_llama().cuda(), data, LINEARS, ["model.embed_tokens"], "model.layers", str(builds[method]),
                             device="cuda:0")
        errors = est.estimate()[-1]
        total[method] = {}
        for n in builds["names"]:
            for f, e in zip(est.levels[n], errors[n]):
                total[method][f] = total[method].get(f, 0.0) + float(e)
        print(f"summed layer error, level_db_iq4_method={method}: " + ", ".join(f"{f} {v:.4g}" for f, v in sorted(total[method].items())))
    xs = [f for f in total["rtn"] if "IQ4_XS" in f]
    assert len(xs) == 1 and total["gptq"][xs[0]] < total["rtn"][xs[0]]


def test_consumers_take_the_walks_levels(builds, tmp_path):
    import copy
    from gptq_gguf_toolkit_amd import evo_quant_search as E
    from gptq_gguf_toolkit_amd import level_db as ldb
    from gptq_gguf_toolkit_amd.gguf_stitcher import stitch_search_result
    from gptq_gguf_toolkit_amd.gguf_writer import parse_gguf
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    names, db = builds["names"], str(builds["gptq"])
    dense_model, packed_model = copy.deepcopy(builds["model"]), copy.deepcopy(builds["model"])
    dense, packed = LevelStore(dense_model, db, "cuda", names), LevelStore(packed_model, db, "cuda", names, resident="packed")
    for key, t in ((4.25, XS), (4.56, NL)):
        state = {n: key for n in names}
        assert dense.switch(state) == 14 and packed.switch(state) == 14
        for n in names:
            want = ldb.load_level(ldb.find_level_file(ldb.layer_dir(db, n), key), "cuda", db)
            assert torch.equal(dense_model.get_submodule(n).weight.data.view(torch.int16), want.view(torch.int16)), (n, key)
            m = packed_model.get_submodule(n)
            assert type(m) is PackedLinear and m.q_type == t
            assert torch.equal(m.dense_weight().view(torch.int16), want.view(torch.int16)), (n, key)
    widths = [4.25, 4.5, 4.56, 2.5625]
    assignment = {n: widths[i % 4] for i, n in enumerate(names)}
    levels = E.scan_available_bitwidths(db, names)
    cfg = tmp_path / E.configuration_name("kl", 4.3)
    cfg.write_text(E.configuration_text([names], [[assignment[n] for n in names]], levels))
    out = stitch_search_result(db, str(cfg), str(tmp_path / "mixed.gguf"), verify=True)
    types = [t[2] for t in parse_gguf(str(out))[1]]
    assert types.count(XS) == sum(v == 4.25 for v in assignment.values()) >= 3
    assert types.count(NL) == sum(v == 4.56 for v in assignment.values()) >= 3
