"""-m gpu: K15, the inverse of the bit-packers -- gq_unpack / gq_dequantize_blocks, gguf_loader and the splitter's HF side.
Every equality is on bits.  Anchors: the reference's own packer / dequantizer outputs (goldens G6-G9), the independent
ggml-layout decoder tests/ggml_spec.py, and the package's own pack / dequantize kernels (already pinned to the reference).
Measured wall time of this file on an MI355X: 8.6 s (5.6 s of it the quantize -> convert fixture)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from ggml_spec import TS, unpack as spec_unpack

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

TYPES = {"Q2_K": 10, "Q3_K": 11, "Q4_K": 12, "Q5_K": 13, "Q6_K": 14}
GROUP = {10: 16, 11: 16, 12: 32, 13: 32, 14: 16}
D_AT = {10: (80, 82), 11: (108,), 12: (0, 2), 13: (0, 2), 14: (208,)}  # byte offsets of the fp16 fields of a block
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from gptq_gguf_toolkit_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u16(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def assert_fields(got, q, d, s, dmin=None, m=None):
    gq, gd, gs, gdmin, gm = got
    assert np.array_equal(gq.cpu().numpy().astype(np.int32), np.asarray(q).astype(np.int32))
    assert np.array_equal(u16(gd), np.asarray(d).astype(np.uint16))
    assert np.array_equal(gs.cpu().numpy().astype(np.int32), np.asarray(s).astype(np.int32))
    if dmin is not None:
        assert np.array_equal(u16(gdmin), np.asarray(dmin).astype(np.uint16))
        assert np.array_equal(gm.cpu().numpy().astype(np.int32), np.asarray(m).astype(np.int32))


def formula_f32(q_type, fields):
    """ds = f32(d) * f32(sc), dm = f32(dmin) * f32(mn), w = ds * f32(code) - dm in numpy fp32 (one rounding per operation)."""
    codes, d, sc, dmin, mn = fields
    G = GROUP[q_type]
    f = lambda bits: np.ascontiguousarray(bits).astype(np.uint16).view(np.float16).astype(np.float32)  # noqa: E731
    ds = np.repeat(f(d), 256 // G, axis=1) * sc.astype(np.float32)
    dm = np.repeat(f(dmin), 256 // G, axis=1) * mn.astype(np.float32)
    return np.repeat(ds, G, axis=1) * codes.astype(np.float32) - np.repeat(dm, G, axis=1)


def random_blocks(q_type, R, nb, seed):
    """Uniformly random bytes; the fp16 d / dmin fields forced finite (exponent 31 -> 30), nothing else restricted."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, size=(R * nb, TS[q_type]), dtype=np.uint8)
    for off in D_AT[q_type]:
        hi = b[:, off + 1]
        hi[(hi & 0x7C) == 0x7C] &= 0xFB
    return b.reshape(R, nb * TS[q_type])


# ------------------------------------------------------------------------------------------------ 5: reference goldens
@pytest.mark.parametrize("name", list(TYPES))
def test_unpack_and_decode_reference_goldens(ops, name):
    g, t = load_golden("g8_g9_rtn_dequant"), TYPES[name]
    packed = dev(g[f"{name}_packed"])
    ksearch = t in (10, 12, 13)
    assert_fields(ops.unpack(t, packed), g[f"{name}_q"], g[f"{name}_d"], g[f"{name}_s"],
                  g[f"{name}_dmin"] if ksearch else None, g[f"{name}_m"] if ksearch else None)
    deq = ops.dequantize_blocks(t, packed, torch.float32)
    assert np.array_equal(deq.cpu().numpy().view(np.uint32), g[f"{name}_deq"].view(np.uint32))


def test_unpack_gptq_step_goldens(ops):
    g = load_golden("g6_g7_step_and_pack")
    tags = [k[:-len("_packed")] for k in g.files if k.endswith("_packed")]
    assert len(tags) == 7
    for tag in tags:
        t = next(v for k, v in TYPES.items() if f"_{k}_" in tag)
        ksearch = t in (10, 12, 13)
        assert_fields(ops.unpack(t, dev(g[f"{tag}_packed"])), g[f"{tag}_q"], g[f"{tag}_d"], g[f"{tag}_s"],
                      g[f"{tag}_dmin"] if ksearch else None, g[f"{tag}_m"] if ksearch else None)


# ------------------------------------------------------------------------------------------------ 6: totality
@pytest.mark.parametrize("nb", [9, 8])
@pytest.mark.parametrize("name", list(TYPES))
def test_decoder_is_total_on_random_bytes(ops, name, nb):
    t, R = TYPES[name], 520  # 4680 / 4160 blocks; 520 * 9 is not a multiple of the 16 blocks a workgroup takes per turn
    b = random_blocks(t, R, nb, seed=1000 * t + nb)
    fields = spec_unpack(t, b)
    blocks = dev(b)
    got = ops.unpack(t, blocks)
    assert_fields(got, *fields)
    assert torch.equal(ops.pack(t, *got), blocks)
    want = formula_f32(t, fields)
    assert np.isfinite(want).all()
    for dt in DTYPES:
        out = ops.dequantize_blocks(t, blocks, dt)
        assert torch.equal(bits(out).cpu(), bits(torch.from_numpy(want).to(dt))), (name, dt)
        assert torch.equal(bits(out), bits(ops.dequantize(t, *got, out_dtype=dt))), (name, dt)
    if t in (10, 12, 13):  # d up to 65504 x scale 63 x code 31 overflows fp16: the infinities are part of the comparison
        assert torch.isinf(ops.dequantize_blocks(t, blocks, torch.float16)).any()


# ------------------------------------------------------------------------------------------------ 7: row_src
@pytest.mark.parametrize("name", list(TYPES))
def test_row_src_is_a_row_gather(ops, name):
    from gptq_gguf_toolkit_amd.gguf_loader import unpermute, unpermute_rows
    t, R, nb = TYPES[name], 1024, 3  # 32 heads x 32 rows
    blocks = dev(random_blocks(t, R, nb, seed=77 + t))
    plain = ops.dequantize_blocks(t, blocks, torch.float16)
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(5)).to(torch.int32).cuda()
    assert torch.equal(ops.dequantize_blocks(t, blocks, torch.float16, perm).view(torch.int16), plain[perm.long()].view(torch.int16))
    rows = unpermute_rows(R, 32, 8).cuda()
    got = ops.dequantize_blocks(t, blocks, torch.float16, rows)
    assert torch.equal(got.view(torch.int16), unpermute(plain, 32, 8).view(torch.int16))
    assert not torch.equal(got.view(torch.int16), plain.view(torch.int16))


# ------------------------------------------------------------------------------------------------ 8: real shapes
@pytest.mark.parametrize("name,R,C", [("Q4_K", 4096, 14336), ("Q6_K", 128256, 4096)])
def test_real_shapes_round_trip_and_guard_rows(ops, name, R, C):
    from gptq_gguf_toolkit_amd import _cabi
    t = TYPES[name]
    torch.manual_seed(8)
    W = torch.randn(R, C, device="cuda", dtype=torch.float16) * 0.02
    x = ops.rtn_quantize(W, t)
    del W
    packed = ops.pack(t, *x)
    back = ops.unpack(t, packed)
    for a, b in zip(back, x):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8) if a.dtype != torch.float16 else a.view(torch.int16),
                                                  b.view(torch.uint8) if b.dtype != torch.float16 else b.view(torch.int16))
    del back
    for dt in (torch.float16, torch.float32):
        want = ops.dequantize(t, *x, out_dtype=dt)
        buf = torch.full((R + 2, C), 0, dtype=dt, device="cuda")  # a guard row before and after `out`
        iv = torch.int16 if dt == torch.float16 else torch.int32
        sentinel = 0x5A5A if dt == torch.float16 else 0x5A5A5A5A
        buf.view(iv).fill_(sentinel)
        out = buf[1:R + 1]
        _cabi.check(_cabi.lib().gq_dequantize_blocks(t, ctypes.c_void_p(packed.data_ptr()), R, C, ctypes.c_void_p(0),
                                                     ctypes.c_void_p(out.data_ptr()), ops._DT[dt],
                                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                    "gq_dequantize_blocks")
        assert torch.equal(out.view(iv), want.view(iv))
        assert bool((buf[0].view(iv) == sentinel).all()) and bool((buf[R + 1].view(iv) == sentinel).all())
        del want, buf, out


# ------------------------------------------------------------------------------------------------ 9, 10: the file
@pytest.fixture(scope="module")
def gguf_model(tmp_path_factory):
    """A 2-layer random Llama (hidden 256, intermediate 512, 4 / 2 heads, vocab 512), mixed K-quant types over the
    projections, embed and lm_head quantized: Quantizer.quantize -> convert -> .gguf."""
    from pathlib import Path
    from make_golden_shim import MIXED, tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import convert
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    from gptq_gguf_toolkit_amd.quantizer import Quantizer
    tmp = tmp_path_factory.mktemp("decode")
    hf, sd = tmp / "hf", tmp / "q"
    model = tiny_llama(dtype=torch.float16).cuda()
    model.save_pretrained(str(hf), safe_serialization=True)
    data = [([], {"input_ids": ids}) for ids in tiny_calib()]
    Quantizer(model, data_loader=data, quantizable_modules=r".*layers.*((q|k|v|o|gate|up|down)_proj)$",
              quantizer_kwargs=dict(rel_damp=0.01, block_size=128, act_order=False, quant_scale="absmax", static_groups=False,
                                    rmin=-1.0, rdelta=0.1, nstep=20, verbose=False),
              pre_block_modules=["model.embed_tokens"], block_modules="model.layers", post_block_modules=["lm_head"],
              quant_non_block_modules=True, device="cuda:0", save_dir=str(sd)).quantize({k: T[v] for k, v in MIXED.items()})
    torch.cuda.synchronize()
    out = convert(Path(hf), Path(sd), tmp / "m.gguf", "f16", vocab=False)
    return model, str(out)


def test_gguf_file_loads_back_to_the_live_model(gguf_model):
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd import gguf_loader
    model, path = gguf_model
    live = model.state_dict()
    sd = gguf_loader.load_state_dict(path, "cuda:0", torch.float16)
    assert set(sd) == set(live)
    for k, w in live.items():
        assert sd[k].dtype == w.dtype and sd[k].shape == w.shape, k
        assert torch.equal(sd[k].view(torch.int16), w.view(torch.int16)), \
            f"{k}: {(sd[k].view(torch.int16) != w.view(torch.int16)).float().mean().item():.3%} of the weights differ"
    # GGUF layout: attn_q / attn_k rows stay permuted, the names are the file's
    raw = dict(gguf_loader.iter_gguf_tensors(path, "cuda:0", torch.float16, hf_layout=False))
    assert "blk.0.attn_q.weight" in raw and not torch.equal(raw["blk.0.attn_q.weight"], live["model.layers.0.self_attn.q_proj.weight"])
    assert torch.equal(gguf_loader.unpermute(raw["blk.1.attn_k.weight"], 4, 2), live["model.layers.1.self_attn.k_proj.weight"])
    fresh = tiny_llama(seed=123, dtype=torch.float16).cuda()
    gguf_loader.load_into_model(fresh, path)
    ids = tiny_calib()[0].cuda()
    with torch.no_grad():
        assert torch.equal(fresh(ids).logits, model(ids).logits)


def test_hf_layers_split_end_to_end(gguf_model, tmp_path):
    from gptq_gguf_toolkit_amd import gguf_splitter
    model, path = gguf_model
    out = tmp_path / "split"
    gguf_splitter.main([path, str(out), "--hf-layers", "--dtype", "float16"])
    man = json.loads((out / "manifest.json").read_text())
    assert man["mapping_stats"] == {"total_layers": 14, "mapped_layers": 14, "unmapped_layers": 0}
    assert set(man["model_info"]) == {"original_file", "dtype", "bitwidth", "use_exact_bitwidth", "split_timestamp"}
    mapping = json.loads((out / "hf_to_gguf_mapping.json").read_text())
    assert len(mapping) == 14 and mapping["model.layers.1.mlp.down_proj.weight"] == "blk.1.ffn_down.weight"
    bits = {"q_proj": "3-Q3_K", "k_proj": "2-Q2_K", "v_proj": "4-Q4_K", "o_proj": "5-Q5_K", "gate_proj": "6-Q6_K",
            "down_proj": "3-Q3_K", "up_proj": "4-Q4_K"}
    live = model.state_dict()
    for name, rec in man["layers"].items():
        assert set(rec) == {"original_name", "gguf_mapped_name", "layer_directory", "dims", "bitwidth", "filename",
                            "metadata_filename", "dtype", "size_bytes", "shape", "n_elements"}
        d = out / name.replace(".weight", "")
        prefix = bits[name.split(".")[-2]]
        assert rec["filename"] == f"{prefix}.pth" and rec["dtype"] == "torch.float16"
        t = torch.load(d / f"{prefix}.pth", weights_only=True)
        assert t.dtype == torch.float16 and torch.equal(t.view(torch.int16), live[name].cpu().view(torch.int16)), name
        meta = json.loads((d / f"{prefix}-metadata.json").read_text())
        assert set(meta["tensor_info"]) == {"name", "gguf_mapped_name", "bitwidth", "dtype", "shape", "n_elements", "n_bytes",
                                            "data_filename", "requires_grad"}
        assert meta["gguf_info"]["quantization"] == prefix.split("-")[1] and meta["tensor_info"]["gguf_mapped_name"] == rec["gguf_mapped_name"]
    assert len(man["layers"]) == 14
