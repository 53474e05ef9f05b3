"""-m gpu: the IQ4_NL / IQ4_XS encoder gq_quantize_iq4 (include/gptq_gguf_iq4_encode.h) against its host form
gguf_writer.quantize_iq4, byte for byte -- which tests/test_iq4_encode_cpu.py holds against the element-by-element contract
(tests/iq4_encode_spec.py) --; and the calibration-weighted IQ4 levels of the one-pass level build with their consumers
(LevelStore in both residencies, the stitcher).

The kernel takes a tile of 256 32-value blocks per workgroup turn.  The shapes:
  IQ4_XS [5, 512]     80 blocks: one partial tile        IQ4_NL [5, 96]      15 blocks: a partial tile that straddles rows
  IQ4_XS [33, 768]   792 blocks: three full tiles that straddle rows (24 blocks a row) and a rest of 24
  IQ4_NL [67, 288]   603 blocks: two full tiles (9 blocks a row, an odd count) and a rest of 91
  both   [130, 1024] 4160 blocks: 16 full tiles and a rest of 64 -- more than one workgroup per row band
  IQ4_NL [8200, 4096] bf16: 4100 tiles, more than the 4096 workgroups of a launch, so some take a second turn (checked
  against the same kernel on the two halves, which take one turn each: results never depend on the launch)."""
import copy
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import iq4_encode_spec as S  # noqa: E402
import iq4_spec  # noqa: E402

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
AS_INT = {4: torch.int32, 2: torch.int16, 1: torch.uint8}
NL, XS = S.NL, S.XS
STEM = {XS: "4.25-IQ4_XS", NL: "4.56-IQ4_NL"}


def bits(t):
    return t.contiguous().view(AS_INT[t.element_size()])


@pytest.fixture(scope="module")
def ops():
    from gptq_gguf_toolkit_amd import ops
    return ops


def host(x: torch.Tensor, t, imp=None) -> np.ndarray:
    from gptq_gguf_toolkit_amd.gguf_writer import quantize_iq4
    return quantize_iq4(x.float().cpu().numpy(), t, None if imp is None else imp.float().cpu().numpy())


# ------------------------------------------------------------------------------------------------ kernel == host form
SHAPES = [(XS, 5, 512), (XS, 33, 768), (XS, 130, 1024), (NL, 5, 96), (NL, 67, 288), (NL, 130, 1024)]


@pytest.mark.parametrize("t,R,C", SHAPES)
def test_kernel_equals_the_host_form_byte_for_byte(ops, t, R, C):
    x32 = torch.from_numpy(S.random_matrix(R, C, seed=t + R + C))
    imp = torch.from_numpy(S.random_importance(C, seed=R)).cuda()
    rows = torch.randperm(R, generator=torch.Generator().manual_seed(R)).to(torch.int32).cuda()
    bs, ts = S.GEOMETRY[t]
    for dt in (F32, F16, BF16):
        x = x32.to(dt).cuda()
        want = {w: host(x, t, imp if w else None) for w in (False, True)}  # (one host encode per weighting, shared below)
        for weighted in (False, True):
            got = ops.quantize_iq4(x, t, imp if weighted else None)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (R, C // bs * ts)
            assert got.cpu().numpy().tobytes() == want[weighted].tobytes(), (dt, weighted)
            got = ops.quantize_iq4(x, t, imp if weighted else None, rows)
            assert got.cpu().numpy().tobytes() == want[weighted][rows.cpu().long().numpy()].tobytes(), (dt, weighted, "rows")
    # decode(encode(x)) through the kernel pair is the spec decoder's, bit for bit
    blocks = ops.quantize_iq4(x32.cuda(), t, imp)
    back = ops.dequantize_blocks(t, blocks, F32)
    assert np.array_equal(back.cpu().numpy().view(np.uint32), iq4_spec.decode(t, blocks.cpu().numpy()).view(np.uint32))


@pytest.mark.parametrize("t", [XS, NL])
def test_kernel_on_the_crafted_blocks(ops, t):
    x, imp = S.crafted(t)
    xd, impd = torch.from_numpy(x).cuda(), torch.from_numpy(imp).cuda()
    for weighted in (False, True):
        got = ops.quantize_iq4(xd, t, impd if weighted else None).cpu().numpy()
        assert got.tobytes() == host(xd, t, impd if weighted else None).tobytes(), weighted
        assert np.isfinite(iq4_spec.decode(t, got)).all()
        ts = S.GEOMETRY[t][1]
        b = got.reshape(x.shape[0], -1, ts)
        assert (b[:2, :, ts - S.GEOMETRY[t][0] // 2:] == 0x88).all()  # all zero, amax = 1e-20: code 8 everywhere
        if t == XS:
            ls = S.xs_scales(got).reshape(x.shape[0], -1, 8)
            assert 0 <= ls.min() and ls.max() <= 63 and ls[4, 0].tolist() == [32, 32, 0, 32, 32, 32, 32, 32]


@pytest.mark.parametrize("t,R,C", [(XS, 5, 512), (NL, 5, 96), (NL, 67, 288)])
def test_nothing_outside_the_blocks_is_written(ops, t, R, C):
    """The library call on a buffer of its own: 64 guard bytes on either side of the blocks stay as they were (the last tile
    ends on a partial 16-byte chunk for [5, 96]: 270 bytes, and for [67, 288]: 10854)."""
    from gptq_gguf_toolkit_amd import _cabi
    bs, ts = S.GEOMETRY[t]
    n = R * C // bs * ts
    x = torch.from_numpy(S.random_matrix(R, C, seed=3)).cuda()
    buf = torch.full((64 + n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    vp = ctypes.c_void_p
    rc = _cabi.lib().gq_quantize_iq4(vp(x.data_ptr()), 0, R, C, t, None, None, vp(buf.data_ptr() + 64),
                                     vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:64] == 0xA5).all() and (out[64 + n:] == 0xA5).all()
    assert out[64:64 + n].tobytes() == host(x, t).tobytes()


def test_a_second_turn_of_a_workgroup_gives_what_one_turn_gives(ops):
    g = torch.Generator(device="cuda").manual_seed(11)
    x = (torch.randn(8200, 4096, generator=g, device="cuda") * 0.03).to(BF16)
    imp = torch.rand(4096, generator=g, device="cuda") + 0.01
    whole = ops.quantize_iq4(x, NL, imp)
    assert torch.equal(whole[:4100], ops.quantize_iq4(x[:4100], NL, imp))
    assert torch.equal(whole[4100:], ops.quantize_iq4(x[4100:], NL, imp))
    probe = slice(8190, 8200)  # the rows of the last tiles, against the host form
    assert whole[probe].cpu().numpy().tobytes() == host(x[probe], NL, imp).tobytes()


def test_binding_refusals(ops):
    from gptq_gguf_toolkit_amd import _cabi
    x = torch.zeros(4, 512, device="cuda")
    imp = torch.ones(512, device="cuda")
    with pytest.raises(_cabi.GQError, match="neither IQ4_NL"):
        ops.quantize_iq4(x, 12)
    with pytest.raises(_cabi.GQError, match="C % 256"):
        ops.quantize_iq4(x[:, :288].contiguous(), XS)
    with pytest.raises(_cabi.GQError, match="C % 32"):
        ops.quantize_iq4(x[:, :40].contiguous(), NL)
    with pytest.raises(_cabi.GQError, match="fp32 / fp16 / bf16"):
        ops.quantize_iq4(x.double(), XS)
    big = torch.zeros(4 * 512 + 4, device="cuda")
    off = big[1:1 + 4 * 512].view(4, 512)
    assert off.data_ptr() % 16 == 4
    with pytest.raises(_cabi.GQError, match="16-byte aligned"):
        ops.quantize_iq4(off, XS)
    with pytest.raises(_cabi.GQError, match="importance must be"):
        ops.quantize_iq4(x, XS, imp.cpu())
    with pytest.raises(_cabi.GQError, match="importance must be"):
        ops.quantize_iq4(x, XS, imp[:256])
    with pytest.raises(_cabi.GQError, match="importance must be"):
        ops.quantize_iq4(x, XS, imp.half())
    with pytest.raises(_cabi.GQError, match="row_src"):
        ops.quantize_iq4(x, XS, None, torch.arange(3, dtype=torch.int32, device="cuda"))
    # a misaligned importance view is copied, not refused: the result is the aligned one's
    wide = torch.rand(513, device="cuda")
    assert wide[1:].data_ptr() % 16 == 4
    x = torch.from_numpy(S.random_matrix(4, 512, seed=9)).cuda()
    assert torch.equal(ops.quantize_iq4(x, XS, wide[1:]), ops.quantize_iq4(x, XS, wide[1:].clone()))


# ------------------------------------------------------------------------------------------------ level build and consumers
LINEARS = r".*layers.*((q|k|v|o|gate|up|down)_proj)$"


def _drive(root, tag, model_dir, **kw):
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    from gptq_gguf_toolkit_amd.quantizer import Quantizer
    model = tiny_llama()  # fp32
    if not os.path.isdir(model_dir):
        model.save_pretrained(model_dir)
    model = model.cuda()
    data = [([], {"input_ids": ids}) for ids in tiny_calib()]
    os.makedirs(root / tag, exist_ok=True)
    drv = Quantizer(model, data_loader=data, quantizable_modules=LINEARS,
                    quantizer_kwargs=dict(rel_damp=0.01, block_size=128, act_order=False, quant_scale="absmax",
                                          static_groups=False, rmin=-1.0, rdelta=0.1, nstep=20, verbose=False),
                    pre_block_modules=["model.embed_tokens"], block_modules="model.layers",
                    post_block_modules=["lm_head"], quant_non_block_modules=True, device="cuda:0", save_dir=str(root / tag))
    drv.quantize_levels([T.Q2_K, T.Q4_K], T.Q4_K, level_db=str(root / f"db_{tag}"), level_db_model=str(model_dir),
                        level_db_vocab=False, trees=False, **kw)
    torch.cuda.synchronize()
    return model


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """Two level builds of the tiny Llama (hidden 256, intermediate 512, 2 layers, vocab 512; levels Q2_K and Q4_K, embed and
    lm_head round-to-nearest at the same levels): db_iq4 with level_db_iq4=("IQ4_XS", "IQ4_NL"), db_plain without.  During the first, an independent hook -- a wrapper around
    GPTQ.compute_levels, which the level build enters with the Hessians still undamped -- records diag(H) of every Linear."""
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd.gptq import GPTQ
    root = tmp_path_factory.mktemp("iq4_levels")
    keep = os.environ.get("GQ_SAVE_SLOT_MB")
    os.environ["GQ_SAVE_SLOT_MB"] = "8"  # the tiny model's files: no large staging slots to pin per run
    diag = {}
    inner = GPTQ.compute_levels

    def recording(hs, *a, **kw):
        for h in hs:
            diag.setdefault(id(h.layer), h.H.diagonal().clone())
        return inner(hs, *a, **kw)

    try:
        GPTQ.compute_levels = staticmethod(recording)
        try:
            built = _drive(root, "iq4", root / "model", level_db_iq4=("IQ4_XS", "IQ4_NL"))
        finally:
            GPTQ.compute_levels = staticmethod(inner)
        _drive(root, "plain", root / "model")
    finally:
        if keep is None:
            os.environ.pop("GQ_SAVE_SLOT_MB", None)
        else:
            os.environ["GQ_SAVE_SLOT_MB"] = keep
    model = tiny_llama(dtype=F16).cuda()
    names = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and "layers" in n]
    assert len(names) == 14
    diag = {n: diag[id(built.get_submodule(n))] for n in names}
    return {"root": root, "db": root / "db_iq4", "plain": root / "db_plain", "model_dir": root / "model", "model": model,
            "names": names, "diag": diag, "calib": tiny_calib()}


def _level_files(db):
    return sorted(os.path.relpath(os.path.join(d, f), db) for d, _, fs in os.walk(db) for f in fs if f.endswith(".pth"))


def test_level_build_writes_the_weighted_iq4_levels_of_every_packed_tensor(ops, world):
    from make_golden_shim import tiny_llama
    from gptq_gguf_toolkit_amd import level_db as ldb
    from gptq_gguf_toolkit_amd.gguf_loader import rotary_row_dst
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import map_tensor_name
    db, plain = world["db"], world["plain"]
    manifest, database = json.load(open(db / "manifest.json")), json.load(open(db / "gguf_layer_database.json"))
    plain_manifest = json.load(open(plain / "manifest.json"))
    fresh = tiny_llama().cuda()  # the checkpoint's own fp32 weights: what every block's Linears held when they were encoded
    for n in world["names"]:
        tensor = map_tensor_name(n + ".weight")
        W = fresh.get_submodule(n).weight.detach()
        imp = world["diag"][n]
        assert imp.shape == (W.shape[1],) and bool((imp > 0).all())
        rows = rotary_row_dst(tensor, W.shape[0], 4, 2, W.device)
        assert (rows is not None) == n.endswith(("q_proj", "k_proj"))
        for t in (XS, NL):
            got = np.fromfile(db / tensor / f"{STEM[t]}.pth", np.uint8)
            want = ops.quantize_iq4(W, t, imp, rows).cpu().numpy()
            assert got.tobytes() == want.tobytes(), (tensor, t)
            assert got.tobytes() != ops.quantize_iq4(W, t, None, rows).cpu().numpy().tobytes()  # the Hessian did weigh in
            bw = float(STEM[t].split("-")[0])
            sidecar, level, _ = ldb.level_records(tensor, tuple(W.shape), t, iq4_spec.NAME[t], bw, bw, got.size, STEM[t])
            assert json.load(open(db / tensor / f"{STEM[t]}-metadata.json"))["tensor_info"] == sidecar
            assert manifest["layers"][tensor]["bitwidths"][str(bw)] == level
        # registered before the K-quant levels: the tensor's database record stays its last K-quant level
        assert list(manifest["layers"][tensor]["bitwidths"]) == ["4.25", "4.56", "2.5625", "4.5"]
        kept = {k: v for k, v in manifest["layers"][tensor]["bitwidths"].items() if k not in ("4.25", "4.56")}
        assert kept == plain_manifest["layers"][tensor]["bitwidths"]
    # embed / lm_head have no Hessian: their levels are the unweighted encoding of the checkpoint's weight, rows as they are
    vocab_ends = ["model.embed_tokens", "lm_head"]
    for n in vocab_ends:
        tensor = map_tensor_name(n + ".weight")
        W = fresh.get_submodule(n).weight.detach()
        for t in (XS, NL):
            got = np.fromfile(db / tensor / f"{STEM[t]}.pth", np.uint8)
            assert got.tobytes() == ops.quantize_iq4(W, t).cpu().numpy().tobytes(), (tensor, t)
        assert list(manifest["layers"][tensor]["bitwidths"]) == ["4.25", "4.56", "2.5625", "4.5"]
    assert database == json.load(open(plain / "gguf_layer_database.json"))
    assert list(manifest["layers"]) == list(plain_manifest["layers"]) and manifest["metadata"] == plain_manifest["metadata"]
    # a tensor without K-quant levels gets none; the build without the option writes no such file and the same others
    with_iq4 = _level_files(db)
    new = [f for f in with_iq4 if "IQ4" in f]
    assert new == sorted(f"{map_tensor_name(n + '.weight')}/{STEM[t]}.pth" for n in world["names"] + vocab_ends for t in (XS, NL))
    others = [f for f in with_iq4 if "IQ4" not in f]
    assert others == _level_files(plain) and len(others) == 16 * 2 + 5
    for f in others:
        assert (db / f).read_bytes() == (plain / f).read_bytes(), f
        assert (db / (f[:-4] + "-metadata.json")).read_bytes() == (plain / (f[:-4] + "-metadata.json")).read_bytes(), f


def test_level_store_switches_to_the_new_levels_in_both_residencies(world):
    from gptq_gguf_toolkit_amd import level_db as ldb
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    names, db = world["names"], str(world["db"])
    dense_model, packed_model = copy.deepcopy(world["model"]), copy.deepcopy(world["model"])
    dense, packed = LevelStore(dense_model, db, "cuda", names), LevelStore(packed_model, db, "cuda", names, resident="packed")
    assert all(dense.level_keys(n) == [2.5625, 4.25, 4.5, 4.56] for n in names)
    for key, t in ((4.25, XS), (4.5, 12), (4.56, NL)):
        state = {n: key for n in names}
        assert dense.switch(state) == 14 and packed.switch(state) == 14
        for n in names:
            want = ldb.load_level(ldb.find_level_file(ldb.layer_dir(db, n), key), "cuda", db)
            assert want.dtype == F16 and bool(torch.isfinite(want).all())
            assert torch.equal(bits(dense_model.get_submodule(n).weight.data), bits(want)), (n, key)
            m = packed_model.get_submodule(n)
            assert type(m) is PackedLinear and m.q_type == t
            assert torch.equal(bits(m.dense_weight()), bits(want)), (n, key)
            if t != 12:  # 4 bits of the checkpoint's own weight: within 12 % rms of it (7 .. 8 % on Gaussian data)
                ref = world["model"].get_submodule(n).weight.detach().float()
                rel = float((want.float() - ref).norm() / ref.norm())
                assert rel < 0.12, (n, key, rel)
    assert dense.find("model.layers.0.self_attn.q_proj", 4.25).rows is not None


def test_stitched_file_that_takes_the_new_levels_verifies(world, tmp_path):
    from gptq_gguf_toolkit_amd import evo_quant_search as E
    from gptq_gguf_toolkit_amd.gguf_stitcher import stitch_search_result
    from gptq_gguf_toolkit_amd.gguf_writer import parse_gguf
    names, db = world["names"], str(world["db"])
    widths = [4.25, 4.5, 4.56, 2.5625]
    assignment = {n: widths[(i + i // 7) % 4] for i, n in enumerate(names)}
    assignment["model.layers.0.self_attn.q_proj"], assignment["model.layers.0.self_attn.k_proj"] = 4.25, 4.56
    levels = E.scan_available_bitwidths(db, names)
    cfg = tmp_path / E.configuration_name("kl", 4.3)
    cfg.write_text(E.configuration_text([names], [[assignment[n] for n in names]], levels))
    out = stitch_search_result(db, str(cfg), str(tmp_path / "mixed.gguf"), verify=True)
    types = [t[2] for t in parse_gguf(str(out))[1]]
    assert types.count(XS) == sum(v == 4.25 for v in assignment.values()) >= 3
    assert types.count(NL) == sum(v == 4.56 for v in assignment.values()) >= 3
