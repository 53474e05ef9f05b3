"""-m gpu: Q8_0 as an ordinary level.  The decode turn of gq_dequantize_blocks / gq_level_switch against the torch expression
of the former loader (`d.float() * q.float()`, then `.to(dtype)`), bit for bit; the encoder gq_quantize_q8_0 against
gguf_writer.quantize_q8_0, byte for byte; the loader; the 8.5-bit level of the one-pass level build and its consumers
(LevelStore, ErrorEstimator, evo_quant_search, the stitcher); the converter's GPU producer."""
import copy
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

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
AS_INT = {4: torch.int32, 2: torch.int16, 1: torch.uint8}
Q8, Q4, Q6 = 8, 12, 14


def bits(t):
    return t.contiguous().view(AS_INT[t.element_size()])


@pytest.fixture(scope="module")
def ops():
    from gptq_gguf_toolkit_amd import ops
    return ops


def q8_bytes(R, C, seed):
    """uint8 [R, C/32*34] of random bytes whose d is any FINITE fp16 bit pattern: both signs, subnormals, +-0 included."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, (R * (C // 32), 34), dtype=np.uint8)
    d = rng.integers(0, 1 << 16, R * (C // 32), dtype=np.uint16)
    d = np.where((d & 0x7C00) == 0x7C00, d & 0xBFFF, d).astype(np.uint16)  # inf / NaN -> a finite pattern of the same sign
    d[:: 7] &= 0x83FF   # subnormals (and zeros where the mantissa is zero)
    d[:1] = 0x8000      # -0
    d[-1:] = 0x0000     # +0
    b[:, :2] = d.view(np.uint8).reshape(-1, 2)
    assert np.isfinite(d.view(np.float16)).all()
    return b.reshape(R, -1)


def torch_decode(raw, R, C, rows, dtype):
    """The loader's expression before the kernel existed."""
    b = raw.reshape(-1, 34)
    t = (b[:, :2].contiguous().view(F16).float() * b[:, 2:].contiguous().view(torch.int8).float()).reshape(R, C)
    if rows is not None:
        t = t[rows.long()]
    return t.to(dtype)


# ------------------------------------------------------------------------------------------------ decode
SHAPES = [(1, 32), (1, 4096), (127, 32), (129, 32), (5, 96), (3, 4128), (257, 64)]


@pytest.mark.parametrize("R,C", SHAPES)
def test_decode_equals_the_torch_expression_bit_for_bit(ops, R, C):
    from ggml_spec import q8_0_decode
    host = q8_bytes(R, C, 100 + R + C)
    raw = torch.from_numpy(host).cuda()
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(R)).to(torch.int32).cuda()
    # the same bytes 34 bytes into a larger buffer: 2-byte and not 4-byte aligned
    big = torch.empty(34 + host.size + 30, dtype=torch.uint8, device="cuda").fill_(0xA5)
    big[34:34 + host.size] = raw.view(-1)
    off = big[34:34 + host.size].view(R, -1)
    assert off.data_ptr() % 4 == 2
    for dt in (F32, F16, BF16):
        for rows in (None, perm):
            want = torch_decode(raw, R, C, rows, dt)
            got = ops.dequantize_blocks(Q8, raw, dt, rows)
            assert got.dtype == dt and tuple(got.shape) == (R, C)
            assert torch.equal(bits(got), bits(want)), (dt, rows is not None)
        got = ops.dequantize_blocks(Q8, off, dt, perm)
        assert torch.equal(bits(got), bits(torch_decode(raw, R, C, perm, dt))), (dt, "misaligned")
    spec = q8_0_decode(host.tobytes(), R * C).reshape(R, C)
    assert np.array_equal(ops.dequantize_blocks(Q8, raw, F32).cpu().numpy().view(np.uint32), spec.view(np.uint32))


def test_decode_binding_refusals(ops):
    from gptq_gguf_toolkit_amd import _cabi
    raw = torch.zeros(4, 3 * 34, dtype=torch.uint8, device="cuda")
    with pytest.raises(_cabi.GQError, match="uint8"):
        ops.dequantize_blocks(Q8, raw[:, :100])
    dst = torch.empty(4, 96, dtype=F16, device="cuda")
    with pytest.raises(_cabi.GQError, match="408 uint8"):
        ops.level_switch([(raw.view(-1)[:400], dst, Q8, None)])
    with pytest.raises(_cabi.GQError, match="uint8"):
        ops.level_switch([(raw, torch.empty(4, 80, dtype=F16, device="cuda"), Q8, None)])


# ------------------------------------------------------------------------------------------------ switch
def test_one_switch_call_mixes_q8_0_with_k_quants_and_a_dense_job(ops):
    g = torch.Generator().manual_seed(5)
    W = (torch.randn(64, 512, generator=g) * 0.05).cuda()
    q4, q6 = ops.pack(Q4, *ops.rtn_quantize(W, Q4)), ops.pack(Q6, *ops.rtn_quantize(W[:33].contiguous(), Q6))
    a = torch.from_numpy(q8_bytes(37, 96, 1)).cuda()       # gathered, C / 32 = 3: turns straddle rows
    b = torch.from_numpy(q8_bytes(129, 32, 2)).cuda()      # one block more than a turn
    rows_a = torch.randperm(37, generator=g).to(torch.int32).cuda()
    rows_6 = torch.randperm(33, generator=g).to(torch.int32).cuda()
    dense = torch.randn(9, 40, generator=g).cuda()

    def fresh():
        return [torch.full(s, float("nan"), dtype=dt, device="cuda")
                for s, dt in (((37, 96), F16), ((64, 512), BF16), ((129, 32), F32), ((33, 512), F16), ((9, 40), F16))]

    d = fresh()
    ops.level_switch([(a, d[0], Q8, rows_a), (q4, d[1], Q4, None), (b, d[2], Q8, None), (q6, d[3], Q6, rows_6),
                      (dense, d[4], None, None)])
    assert torch.equal(bits(d[0]), bits(ops.dequantize_blocks(Q8, a, F16, rows_a)))
    assert torch.equal(bits(d[0]), bits(torch_decode(a, 37, 96, rows_a, F16)))
    assert torch.equal(bits(d[1]), bits(ops.dequantize_blocks(Q4, q4, BF16)))
    assert torch.equal(bits(d[2]), bits(ops.dequantize_blocks(Q8, b, F32)))
    assert torch.equal(bits(d[3]), bits(ops.dequantize_blocks(Q6, q6, F16, rows_6)))
    assert torch.equal(bits(d[4]), bits(dense.to(F16)))
    e = fresh()  # the K-quant and dense jobs alone give the same
    ops.level_switch([(q4, e[1], Q4, None), (q6, e[3], Q6, rows_6), (dense, e[4], None, None)])
    for k in (1, 3, 4):
        assert torch.equal(bits(d[k]), bits(e[k])), k


# ------------------------------------------------------------------------------------------------ encode
def host_encode(x: torch.Tensor) -> np.ndarray:
    from gptq_gguf_toolkit_amd.gguf_writer import quantize_q8_0
    with np.errstate(over="ignore"):
        return quantize_q8_0(x.float().cpu().numpy())


def test_encode_crafted_blocks(ops):
    import q8_cases as Q
    x = torch.from_numpy(Q.crafted_encoder_matrix()).cuda()
    got = ops.quantize_q8_0(x).cpu().numpy()
    assert got.shape == (4, 34) and got.dtype == np.uint8
    assert got[0, 2:11].view(np.int8).tolist() == Q.HALVES_AWAY  # roundf: half away from zero, not to even
    assert not got[1].any()
    d = got[:, :2].copy().view(np.float16).ravel()
    assert np.isinf(d[2]) and 0 < d[3] < np.float16(6.104e-5)
    assert got.tobytes() == host_encode(x).tobytes()


@pytest.fixture(scope="module")
def random_x():
    import q8_cases as Q
    x = Q.random_encoder_matrix()
    assert Q.division_and_reciprocal_differ(x).size >= 1  # the input does tell x * (1 / d) from x / d
    return torch.from_numpy(x)


def test_encode_random_data_in_every_input_dtype(ops, random_x):
    for dt in (F32, F16, BF16):
        x = random_x.to(dt).cuda()
        got = ops.quantize_q8_0(x)
        assert tuple(got.shape) == (2048, 1024 // 32 * 34)
        assert got.cpu().numpy().tobytes() == host_encode(x).tobytes(), dt


@pytest.mark.parametrize("R,C", [(1, 32), (3, 96), (5, 4128), (2048, 1024)])
def test_encode_shapes_and_the_row_gather(ops, random_x, R, C):
    x = random_x.reshape(-1)[:R * C].reshape(R, C).contiguous().cuda()
    rows = torch.randperm(R, generator=torch.Generator().manual_seed(R)).to(torch.int32).cuda()
    assert ops.quantize_q8_0(x).cpu().numpy().tobytes() == host_encode(x).tobytes()
    assert ops.quantize_q8_0(x, rows).cpu().numpy().tobytes() == host_encode(x[rows.long()]).tobytes()
    # decode(encode(x)) through the kernel pair is the host pair's
    back = ops.dequantize_blocks(Q8, ops.quantize_q8_0(x), F32)
    assert torch.equal(bits(back), bits(torch_decode(torch.from_numpy(host_encode(x)).cuda(), R, C, None, F32)))


# ------------------------------------------------------------------------------------------------ loader
def test_loader_decodes_q8_0_with_the_rotary_rows_folded_in(ops, tmp_path):
    from gptq_gguf_toolkit_amd.gguf_loader import iter_gguf_tensors, unpermute_rows
    from gptq_gguf_toolkit_amd.gguf_writer import GGMLType, GGUFWriter
    w = GGUFWriter(str(tmp_path / "q8.gguf"), "llama")
    w.add_uint32("llama.attention.head_count", 4)
    w.add_uint32("llama.attention.head_count_kv", 2)
    aq, emb = q8_bytes(64, 96, 11), q8_bytes(40, 64, 12)
    norm = np.random.default_rng(3).random(96, dtype=np.float32)
    w.add_tensor("blk.0.attn_q.weight", aq, raw_dtype=GGMLType.Q8_0)
    w.add_tensor("token_embd.weight", emb, raw_dtype=GGMLType.Q8_0)
    w.add_tensor("output_norm.weight", norm)
    w.write()
    rows = unpermute_rows(64, 4, 4).cuda()
    assert not torch.equal(rows.cpu(), torch.arange(64, dtype=torch.int32))
    for dt in (None, F16):
        sd = dict(iter_gguf_tensors(str(tmp_path / "q8.gguf"), "cuda:0", dt))
        eff = dt or F32
        assert sd["model.layers.0.self_attn.q_proj.weight"].dtype == eff
        assert torch.equal(bits(sd["model.layers.0.self_attn.q_proj.weight"]),
                           bits(torch_decode(torch.from_numpy(aq).cuda(), 64, 96, rows, eff)))
        assert torch.equal(bits(sd["model.embed_tokens.weight"]), bits(torch_decode(torch.from_numpy(emb).cuda(), 40, 64, None, eff)))
        assert torch.equal(sd["model.norm.weight"].cpu(), torch.from_numpy(norm).to(eff))
    stored = dict(iter_gguf_tensors(str(tmp_path / "q8.gguf"), "cuda:0", None, hf_layout=False, quant_dtype=F16))
    assert stored["blk.0.attn_q.weight"].dtype == F32  # quant_dtype is the K-quants' alone
    assert torch.equal(bits(stored["blk.0.attn_q.weight"]), bits(torch_decode(torch.from_numpy(aq).cuda(), 64, 96, None, F32)))


# ------------------------------------------------------------------------------------------------ level build and consumers
LINEARS = r".*layers.*((q|k|v|o|gate|up|down)_proj)$"
STEM = "8.5-Q8_0"


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
                    post_block_modules=["lm_head"], quant_non_block_modules=False, device="cuda:0", save_dir=str(root / tag))
    drv.quantize_levels([T.Q2_K, T.Q4_K], T.Q4_K, level_db=str(root / f"db_{tag}"), level_db_model=str(model_dir),
                        level_db_vocab=False, trees=False, **kw)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """Two level builds of the tiny Llama (hidden 256, 2 layers, vocab 512; levels Q2_K and Q4_K): db_q8 with
    level_db_q8_0, db_plain without."""
    from make_golden_shim import tiny_calib, tiny_llama
    root = tmp_path_factory.mktemp("q8_levels")
    keep = os.environ.get("GQ_SAVE_SLOT_MB")
    os.environ["GQ_SAVE_SLOT_MB"] = "8"  # the tiny model's files: no large staging slots to pin per run
    try:
        _drive(root, "q8", root / "model", level_db_q8_0=True)
        _drive(root, "plain", root / "model")
    finally:
        if keep is None:
            os.environ.pop("GQ_SAVE_SLOT_MB", None)
        else:
            os.environ["GQ_SAVE_SLOT_MB"] = keep
    model = tiny_llama(dtype=F16).cuda()
    names = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and "layers" in n]
    assert len(names) == 14
    torch.save(tiny_calib(), str(root / "calib.pt"))
    return {"root": root, "db": root / "db_q8", "plain": root / "db_plain", "model_dir": root / "model", "model": model,
            "names": names, "calib": tiny_calib()}


def _level_files(db):
    return sorted(os.path.relpath(os.path.join(d, f), db) for d, _, fs in os.walk(db) for f in fs if f.endswith(".pth"))


def test_level_build_writes_the_q8_0_level_of_every_packed_tensor(world):
    from safetensors import safe_open
    from gptq_gguf_toolkit_amd import level_db as ldb
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import map_tensor_name, permute
    db, plain = world["db"], world["plain"]
    manifest, database = json.load(open(db / "manifest.json")), json.load(open(db / "gguf_layer_database.json"))
    with safe_open(str(world["model_dir"] / "model.safetensors"), framework="pt", device="cpu") as f:
        for n in world["names"]:
            tensor = map_tensor_name(n + ".weight")
            W = f.get_tensor(n + ".weight")
            if n.endswith("q_proj"):
                W = permute(W, 4, 4)
            elif n.endswith("k_proj"):
                W = permute(W, 4, 2)
            got = np.fromfile(db / tensor / f"{STEM}.pth", np.uint8)
            assert got.tobytes() == host_encode(W).tobytes(), tensor  # RTN of the unmodified weight, in GGUF row order
            sidecar, level, record = ldb.level_records(tensor, tuple(W.shape), 8, "Q8_0", 8.5, 8.5, got.size, STEM)
            assert json.load(open(db / tensor / f"{STEM}-metadata.json"))["tensor_info"] == sidecar
            assert manifest["layers"][tensor]["bitwidths"]["8.5"] == level
            assert list(manifest["layers"][tensor]["bitwidths"]) == ["2.5625", "4.5", "8.5"]
            assert database[tensor] == record
    # a tensor without K-quant levels gets none; the build without the flag writes no such file and the same others
    with_q8 = _level_files(db)
    assert [f for f in with_q8 if STEM in f] == sorted(f"{map_tensor_name(n + '.weight')}/{STEM}.pth" for n in world["names"])
    others = [f for f in with_q8 if STEM not in f]
    assert others == _level_files(plain) and len(others) == 14 * 2 + 5 + 2
    for f in others:
        assert (db / f).read_bytes() == (plain / f).read_bytes(), f
        assert (db / (f[:-4] + "-metadata.json")).read_bytes() == (plain / (f[:-4] + "-metadata.json")).read_bytes(), f


def test_level_store_holds_and_switches_the_q8_0_level(world):
    from gptq_gguf_toolkit_amd import level_db as ldb
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    model, names, db = copy.deepcopy(world["model"]), world["names"], str(world["db"])
    store = LevelStore(model, db, "cuda", names)  # (refused every Q8_0 level before the type was one)
    assert all(store.level_keys(n) == [2.5625, 4.5, 8.5] for n in names)
    numel = sum(model.get_submodule(n).weight.numel() for n in names)
    assert numel * (84 + 144 + 272) // 256 <= store.bytes() <= numel * (84 + 144 + 272) // 256 + 4 * (256 + 128)
    ptrs = {n: model.get_submodule(n).weight.data_ptr() for n in names}
    assert store.switch({n: 4.5 for n in names}) == 14 and store.switch({n: 8.5 for n in names}) == 14
    for n in names:
        lv = store.find(n, 8.5)
        assert lv.kind == 8 and lv.data.dtype == torch.uint8
        ldir = ldb.layer_dir(db, n)
        want = ldb.load_level(os.path.join(ldir, f"{STEM}.pth"), "cuda", db)
        assert want.dtype == F16
        w = model.get_submodule(n).weight
        assert w.data_ptr() == ptrs[n] and torch.equal(bits(w.data), bits(want.to(w.dtype))), n
        assert torch.equal(bits(store.level_tensor(n, 8.5)), bits(want))
        # 8.5 bits of the checkpoint's own weight.  Per value: half a step d <= amax / 127 / 2, plus three roundings of
        # relative size 2^-11 (d to fp16, times up to 127 codes; the fp16 output; the fp16 model weight compared with)
        ref = world["model"].get_submodule(n).weight.detach().float()
        assert float((w.detach().float() - ref).abs().max()) <= float(ref.abs().max()) / 127 * 0.51 + 2e-3 * float(ref.abs().max())
    assert store.find("model.layers.0.self_attn.q_proj", 8.5).rows is not None


def test_error_estimator_reports_the_q8_0_level_below_q2_k(world):
    from gptq_gguf_toolkit_amd.error_estimator import ErrorEstimator
    model = copy.deepcopy(world["model"])
    data = [([], {"input_ids": ids}) for ids in world["calib"][:2]]
    est = ErrorEstimator(model, data, LINEARS, ["model.embed_tokens"], "model.layers", str(world["db"]), device="cuda:0")
    errors = est.estimate()[-1]
    assert sorted(errors) == sorted(world["names"])
    for n in world["names"]:
        assert est.levels[n] == ["2.5625-Q2_K.pth", "4.5-Q4_K.pth", f"{STEM}.pth"]
        q2, q4, q8 = errors[n]
        print(f"    {n}: Q2_K {q2:.3e}  Q4_K {q4:.3e}  Q8_0 {q8:.3e}")
        assert np.isfinite(q8) and 0 <= q8 < q2, n


def test_search_runs_on_a_database_with_a_q8_0_level(world, tmp_path):
    import shutil
    from gptq_gguf_toolkit_amd import evo_quant_search as S
    db = tmp_path / "db"
    shutil.copytree(world["db"], db)  # main() writes its configuration into the database
    calib = str(world["root"] / "calib.pt")
    parent, out = S.main(["--model_name_or_path", str(world["model_dir"]), "--dtype", "float16", "--calibration_data", calib,
                          "--eval_datasets", calib, "--calibration_tokens", "512", "--eval_tokens", "128",
                          "--calibration_sequence_length", "64", "--eval_sequence_length", "64", "--generations", "2",
                          "--offspring", "4", "--target_bitwidth", "5", "--quant_weights_path", str(db),
                          "--survivors_per_selection", "2", "1", "--tokens_per_selection", "128", "256"])
    assert os.path.basename(out) == "evo-kl-configuration-5.0.txt" and os.path.isfile(out)
    lines = open(out).read().splitlines()
    assert len(lines) == 14 and all(": " in ln and ln.endswith(".pth)") for ln in lines)
    assert {bw for group in parent for bw in group} <= {2.5625, 4.5, 8.5} and sum(len(g) for g in parent) == 14


def test_stitched_file_with_q8_0_tensors_verifies_and_loads_to_the_stores_state(world, tmp_path):
    from gptq_gguf_toolkit_amd import evo_quant_search as S, gguf_loader
    from gptq_gguf_toolkit_amd.gguf_stitcher import stitch_search_result
    from gptq_gguf_toolkit_amd.gguf_writer import parse_gguf
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    names, db = world["names"], str(world["db"])
    widths = [2.5625, 4.5, 8.5]
    assignment = {n: widths[(i + i // 7) % 3] for i, n in enumerate(names)}
    assignment["model.layers.0.self_attn.q_proj"], assignment["model.layers.0.self_attn.k_proj"] = 8.5, 4.5
    levels = S.scan_available_bitwidths(db, names)
    cfg = tmp_path / S.configuration_name("kl", 5.0)
    cfg.write_text(S.configuration_text([names], [[assignment[n] for n in names]], levels))
    out = stitch_search_result(db, str(cfg), str(tmp_path / "mixed.gguf"), verify=True)
    types = [t[2] for t in parse_gguf(str(out))[1]]
    assert types.count(8) == sum(v == 8.5 for v in assignment.values()) >= 4
    loaded = gguf_loader.load_into_model(copy.deepcopy(world["model"]), str(out))
    switched = copy.deepcopy(world["model"])
    LevelStore(switched, db, "cuda", names).switch(assignment)
    want = switched.state_dict()
    for k, t in loaded.state_dict().items():
        assert torch.equal(bits(t), bits(want[k])), k


# ------------------------------------------------------------------------------------------------ converter
def test_converter_q8_0_on_the_gpu_writes_the_host_paths_file(ops, tmp_path):
    from safetensors.torch import save_file
    from gptq_gguf_toolkit_amd.gguf_writer import read_gguf
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import convert, permute
    h, V = 256, 48
    cfg = {"architectures": ["LlamaForCausalLM"], "hidden_size": h, "intermediate_size": 336, "num_hidden_layers": 1,
           "num_attention_heads": 4, "num_key_value_heads": 2, "vocab_size": V, "max_position_embeddings": 128,
           "rms_norm_eps": 1e-5, "rope_theta": 10000.0}
    g = torch.Generator().manual_seed(1)
    p = "model.layers.0."
    sd = {"model.embed_tokens.weight": torch.randn(V, h, generator=g), "model.norm.weight": torch.rand(h, generator=g),
          p + "self_attn.q_proj.weight": torch.randn(h, h, generator=g),       # left unquantized: Q8_0 with the q permute
          p + "self_attn.k_proj.weight": torch.randn(h // 2, h, generator=g),  # replaced by a GPTQ result
          p + "mlp.down_proj.weight": torch.randn(h, 336, generator=g),        # 336 % 32 != 0: F16 on the host path
          p + "input_layernorm.weight": torch.rand(h, generator=g), "lm_head.weight": torch.randn(V, h, generator=g)}
    sd = {k: v.to(BF16) for k, v in sd.items()}
    hf = tmp_path / "hf"
    hf.mkdir()
    save_file(sd, str(hf / "model.safetensors"))
    (hf / "config.json").write_text(json.dumps(cfg))
    W = (torch.randn(h // 2, h, generator=g) * 0.05).cuda()
    q, d, s, dmin, m = (t.cpu() for t in ops.rtn_quantize(W, Q4))
    qdir = tmp_path / "q" / "model.layers.0.self_attn.k_proj"
    qdir.mkdir(parents=True)
    torch.save({"q_type": Q4, "qweight": q, "super_group_scale": d, "super_group_zero": dmin, "group_scale_quant": s,
                "group_zero_quant": m}, str(qdir / "data.pth"))
    tm = {}
    convert(hf, tmp_path / "q", tmp_path / "a.gguf", "q8_0", vocab=False, pipelined=True, timing=tm)
    convert(hf, tmp_path / "q", tmp_path / "b.gguf", "q8_0", vocab=False, pipelined=False)
    assert (tmp_path / "a.gguf").read_bytes() == (tmp_path / "b.gguf").read_bytes()
    assert "q8_0" in tm  # the GPU producer ran
    _, ts = read_gguf(str(tmp_path / "a.gguf"))
    assert ts["blk.0.attn_q.weight"][1] == 8 and ts["token_embd.weight"][1] == 8 and ts["output.weight"][1] == 8
    assert ts["blk.0.ffn_down.weight"][1] == 1 and ts["blk.0.attn_k.weight"][1] == Q4 and ts["output_norm.weight"][1] == 0
    want = host_encode(permute(sd[p + "self_attn.q_proj.weight"], 4, 4))
    assert ts["blk.0.attn_q.weight"][2].tobytes() == want.tobytes()
