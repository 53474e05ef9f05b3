"""CPU: the configuration converter against the reference's own run (G20) and the stitcher on databases made by this
package's writer and splitter from random bytes -- a "tensor" here is a correctly sized payload, nothing is decoded.  The
stitched files are read back by the independent spec readers (tests/gguf_spec_reader.py for the key/value data, read_tensors
below for the tensor infos and payloads), never by the package's parse_gguf."""
import json
import os
import shutil
import struct

import numpy as np
import pytest

from conftest import GOLDEN
from gguf_spec_reader import read_kv

F32, F16, Q2_K, Q4_K, Q6_K = 0, 1, 10, 12, 14
SIZES = {F32: (1, 4), F16: (1, 2), Q2_K: (256, 84), Q4_K: (256, 144), Q6_K: (256, 210)}  # ggml.h: block values, block bytes
EXACT = {Q2_K: "2.5625-Q2_K", Q4_K: "4.5-Q4_K", Q6_K: "6.5625-Q6_K"}
PROJ = (("attn_q", 4, 256), ("attn_k", 2, 256), ("attn_v", 2, 256), ("attn_output", 4, 256), ("ffn_gate", 8, 256),
        ("ffn_up", 8, 256), ("ffn_down", 4, 512))
SKIPPED = ("general.file_type", "general.quantization_version")


def read_tensors(path):
    """[(name, ggml dims innermost first, ggml type, payload bytes)] in file order, from the GGUF v3 specification: after the
    key/value data come n_tensors x {string name, u32 n_dims, u64 dims[n_dims], u32 type, u64 offset}; the data section
    starts at the next multiple of general.alignment (32 without the key) and the offsets are relative to it."""
    buf = open(path, "rb").read()
    kv, _, n_tensors = read_kv(path)
    scalar = {0: 1, 1: 1, 2: 2, 3: 2, 4: 4, 5: 4, 6: 4, 7: 1, 10: 8, 11: 8, 12: 8}
    pos = 24

    def skip_value(t):
        nonlocal pos
        if t == 8:
            pos += 8 + struct.unpack_from("<Q", buf, pos)[0]
        elif t == 9:
            et, cnt = struct.unpack_from("<IQ", buf, pos)
            pos += 12
            for _ in range(cnt):
                skip_value(et)
        else:
            pos += scalar[t]

    for _ in range(len(kv)):
        skip_value(8)
        t = struct.unpack_from("<I", buf, pos)[0]
        pos += 4
        skip_value(t)
    infos = []
    for _ in range(n_tensors):
        n = struct.unpack_from("<Q", buf, pos)[0]
        name = buf[pos + 8:pos + 8 + n].decode("utf-8")
        pos += 8 + n
        nd = struct.unpack_from("<I", buf, pos)[0]
        dims = struct.unpack_from(f"<{nd}Q", buf, pos + 4)
        gt, off = struct.unpack_from("<IQ", buf, pos + 4 + 8 * nd)
        pos += 4 + 8 * nd + 12
        infos.append((name, tuple(dims), gt, off))
    align = kv.get("general.alignment", 32)
    data0 = (pos + align - 1) // align * align
    out = []
    for name, dims, gt, off in infos:
        bs, ts = SIZES[gt]
        nbytes = int(np.prod(dims)) // bs * ts
        assert off % align == 0 and data0 + off + nbytes <= len(buf), name
        out.append((name, dims, gt, buf[data0 + off:data0 + off + nbytes]))
    assert len(buf) % align == 0
    return out


def write_model(path, proj_types, seed):
    """A small Llama-shaped GGUF of random payload bytes: token_embd (F16), 2 blocks x (attn_norm F32, 7 projections of
    proj_types[i], ffn_norm F32), output_norm (F32), output (Q6_K), and eleven keys of eight value types.  The bytes of the
    projections depend on `seed`; everything else is the same in every file."""
    from gptq_gguf_toolkit_amd.gguf_writer import GGUFValueType as V, GGUFWriter
    w = GGUFWriter(str(path), "llama")
    w.add_string("general.name", "stitch-test")
    w.add_uint32("general.alignment", 32)
    w.add_uint32("llama.block_count", 2)
    w.add_float32("llama.rope.freq_base", 10000.0)
    w.add("llama.some_int64", V.INT64, -5)
    w.add("llama.some_uint64", V.UINT64, 2 ** 40)
    w.add_uint32("general.file_type", 1)
    w.add_bool("tokenizer.ggml.add_bos_token", True)
    w.add_array("tokenizer.ggml.tokens", ["<s>", "a", "b", "é"])
    w.add_array("tokenizer.ggml.scores", [0.0, -1.5, -2.25, -3.0])
    w.add("tokenizer.ggml.token_type", V.ARRAY, [3, 1, 1, 1], V.INT32)
    w.add("llama.some_u16_array", V.ARRAY, [7, 9], V.UINT16)  # an element type gguf-py's inference would not choose
    w.add_uint32("general.quantization_version", 2)
    fixed, rng = np.random.default_rng(1), np.random.default_rng(seed)

    def blocks(r, name, R, C, t):
        w.add_tensor(name, r.integers(0, 256, (R, C // 256 * SIZES[t][1]), dtype=np.uint8), raw_dtype=t)

    w.add_tensor("token_embd.weight", fixed.standard_normal((16, 256)).astype(np.float16))
    for b in range(2):
        w.add_tensor(f"blk.{b}.attn_norm.weight", fixed.standard_normal(256).astype(np.float32))
        for i, (p, R, C) in enumerate(PROJ):
            blocks(rng, f"blk.{b}.{p}.weight", R, C, proj_types[i])
        w.add_tensor(f"blk.{b}.ffn_norm.weight", fixed.standard_normal(256).astype(np.float32))
    w.add_tensor("output_norm.weight", fixed.standard_normal(256).astype(np.float32))
    blocks(fixed, "output.weight", 16, 256, Q6_K)
    w.write()
    return str(path)


def split(path, db):
    from gptq_gguf_toolkit_amd import gguf_splitter
    gguf_splitter.main([path, str(db), "--gguf-layers", "--exact"])


def stitcher(db, out, **kw):
    from gptq_gguf_toolkit_amd.gguf_stitcher import GGUFStitcher
    return GGUFStitcher(str(db), kw.pop("config", None), str(out), **kw)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """uniform: one file (Q4_K attention, Q6_K feed-forward) and its database; mixed: three files (all projections Q2_K,
    Q4_K, Q6_K, different bytes) split into one database."""
    tmp = tmp_path_factory.mktemp("stitch")
    uniform = write_model(tmp / "uniform.gguf", [Q4_K] * 4 + [Q6_K] * 3, seed=2)
    split(uniform, tmp / "udb")
    levels = {t: write_model(tmp / f"level{t}.gguf", [t] * 7, seed=10 + t) for t in (Q2_K, Q4_K, Q6_K)}
    for path in levels.values():
        split(path, tmp / "mdb")
    return {"tmp": tmp, "uniform": uniform, "udb": tmp / "udb", "levels": levels, "mdb": tmp / "mdb"}


# ------------------------------------------------------------------------------------------------ 1: the converter
with open(os.path.join(GOLDEN, "G20_config_convert.json")) as _f:
    G20 = json.load(_f)


@pytest.mark.parametrize("case", sorted(G20))
def test_converter_against_the_reference(case, tmp_path):
    from gptq_gguf_toolkit_amd import config_converter as C
    rec = G20[case]
    assert C.detect_moe_model(rec["input"]) == rec["detected_moe"]
    is_moe = rec["detected_moe"] if rec["is_moe"] is None else rec["is_moe"]
    got = C.convert_hf_to_gguf_config(rec["input"], rec["missing_value"], is_moe)
    assert got == rec["dict"] and list(got) == rec["keys_in_order"]
    C.write_config_file(got, str(tmp_path / "out.txt"))
    assert (tmp_path / "out.txt").read_text() == rec["written"]


def test_converter_cli(tmp_path, capsys):
    from gptq_gguf_toolkit_amd import config_converter as C
    rec = G20["search_result_cli_default"]
    (tmp_path / "in.txt").write_text(rec["input"])
    C.main([str(tmp_path / "in.txt"), "-o", str(tmp_path / "out.txt")])  # the defaults: auto-detection, "32 (32-F32.pth)"
    assert (tmp_path / "out.txt").read_text() == rec["written"]
    capsys.readouterr()
    C.main([str(tmp_path / "in.txt")])
    assert capsys.readouterr().out == rec["written"]
    (tmp_path / "moe.txt").write_text(G20["mixtral_read_as_dense"]["input"])
    C.main([str(tmp_path / "moe.txt"), "--dense", "--missing-value", "32", "-o", str(tmp_path / "dense.txt")])
    assert (tmp_path / "dense.txt").read_text() == G20["mixtral_read_as_dense"]["written"]
    for argv in ([str(tmp_path / "nothing.txt")], [str(tmp_path / "in.txt"), "--moe", "--dense"]):
        with pytest.raises(SystemExit) as e:
            C.main(argv)
        assert e.value.code == 1


# ------------------------------------------------------------------------------------------------ 2: uniform round trip
@pytest.mark.parametrize("with_original", [True, False])
def test_uniform_round_trip(world, tmp_path, with_original):
    from gptq_gguf_toolkit_amd import gguf_stitcher
    out = tmp_path / "out.gguf"
    if not with_original:  # the manifest path: nothing but the database (the splitter recorded the original's file name)
        db = tmp_path / "db"
        shutil.copytree(world["udb"], db)
    else:
        db = world["udb"]
    argv = [str(db), str(out)] + (["--original-model", world["uniform"]] if with_original else [])
    assert gguf_stitcher.main(argv) == 0
    assert out.exists() and not (tmp_path / "out.gguf.partial").exists()
    want, got = read_tensors(world["uniform"]), read_tensors(str(out))
    assert len(want) == 21 and {t for _, _, t, _ in want} == {F32, F16, Q4_K, Q6_K}
    assert [t[:3] for t in got] == [t[:3] for t in want]  # names in order, shapes, types
    for (name, _, _, a), (_, _, _, b) in zip(want, got):
        assert a == b, name
    kv0, types0, _ = read_kv(world["uniform"])
    kv1, types1, _ = read_kv(str(out))
    keep = [k for k in kv0 if k not in SKIPPED]
    assert len(keep) == 12 and len({str(types0[k]) for k in keep}) >= 8
    assert [k for k in kv1 if k not in SKIPPED] == keep and list(kv1)[-2:] == list(SKIPPED)
    for k in keep:
        assert types1[k] == types0[k] and kv1[k] == kv0[k], k
    assert types1["llama.some_u16_array"] == ("array", 2) and types1["general.file_type"] == 4 == types1["general.quantization_version"]
    assert kv1["general.quantization_version"] == 2


def test_manifest_without_types_falls_back_to_inference(world, tmp_path):
    """The reference's manifests carry values only: integers become UINT32, floats FLOAT32, arrays what gguf-py infers."""
    db = tmp_path / "db"
    shutil.copytree(world["udb"], db)
    man = json.loads((db / "manifest.json").read_text())
    for field in man["metadata"].values():
        del field["types"]
    man["model_info"]["original_file"] = "gone.gguf"
    (db / "manifest.json").write_text(json.dumps(man))
    stitcher(db, tmp_path / "o.gguf").stitch_model()
    kv, types, _ = read_kv(str(tmp_path / "o.gguf"))
    assert types["llama.block_count"] == 4 and types["llama.rope.freq_base"] == 6 and types["tokenizer.ggml.add_bos_token"] == 7
    assert types["llama.some_uint64"] == 10 and types["llama.some_int64"] == 5 and types["llama.some_u16_array"] == ("array", 5)
    assert types["tokenizer.ggml.tokens"] == ("array", 8) and kv["tokenizer.ggml.tokens"] == ["<s>", "a", "b", "é"]


# ------------------------------------------------------------------------------------------------ 3: mixed stitch
CONFIG = """# a search result, by hand
blk.0.attn_q.weight: 2.5625 (2.5625-Q2_K.pth)
blk.0.attn_k.weight: 6.5625

a line without a colon
blk.0.attn_v.weight: 4.5 Q4_K
blk.1.ffn_up.weight: 6 Q6_K
blk.1.ffn_down.weight: 3
blk.1.ffn_gate.weight: four
blk.1.attn_q.weight: 6.5625 (6.5625-Q6_K.pth)
blk.1.attn_k.weight:6.5625   Q2_K
blk.1.attn_v.weight: 1 2 3
"""
CHOSEN = {"blk.0.attn_q.weight": Q2_K, "blk.0.attn_k.weight": Q6_K, "blk.0.attn_v.weight": Q4_K, "blk.1.ffn_up.weight": Q6_K,
          "blk.1.ffn_down.weight": Q2_K, "blk.1.attn_q.weight": Q6_K, "blk.1.attn_k.weight": Q6_K}  # 6.5625 Q2_K: the exact width wins


def test_mixed_stitch(world, tmp_path, capsys):
    (tmp_path / "config.txt").write_text(CONFIG)
    st = stitcher(world["mdb"], tmp_path / "mixed.gguf", config=str(tmp_path / "config.txt"), original_model_path=world["levels"][Q4_K])
    warnings = [line for line in capsys.readouterr().out.splitlines() if line.startswith("Warning: Could not parse")]
    assert len(warnings) == 2 and "line 9" in warnings[0] and "line 12" in warnings[1]
    st.stitch_model()
    sources = {t: {n: (dims, gt, raw) for n, dims, gt, raw in read_tensors(p)} for t, p in world["levels"].items()}
    got = read_tensors(str(tmp_path / "mixed.gguf"))
    assert [n for n, *_ in got] == [n for n, *_ in read_tensors(world["levels"][Q4_K])]
    seen = set()
    for name, dims, gt, raw in got:
        level = CHOSEN.get(name, Q4_K)  # unlisted (and unparsable) tensors: the default rule, 4.0 / Q4_K -> 4.5-Q4_K.pth
        assert (dims, gt, raw) == sources[level][name], name
        if ".attn_" in name and "norm" not in name or ".ffn_" in name and "norm" not in name:
            assert gt == level and raw != sources[Q2_K if level != Q2_K else Q4_K][name]
            seen.add(gt)
    assert seen == {Q2_K, Q4_K, Q6_K}


LEVELS = [{"bitwidth": 4.5, "filename": "4.5-Q4_K.pth", "quant_type": "Q4_K"}, {"bitwidth": 4.5, "filename": "4.5-Q4_0.pth", "quant_type": "Q4_0"},
          {"bitwidth": 2.5625, "filename": "2.5625-Q2_K.pth", "quant_type": "Q2_K"}, {"bitwidth": 5.5, "filename": "5.5-Q5_0.pth", "quant_type": "Q5_0"},
          {"bitwidth": 6.5625, "filename": "6.5625-Q6_K.pth", "quant_type": "Q6_K"}, {"bitwidth": 8.0, "filename": "8.pth", "quant_type": None}]


@pytest.mark.parametrize("width,qtype,want", [
    (4.5, "Q4_0", "4.5-Q4_0.pth"),     # exact width and type
    (4.5, "Q6_K", "4.5-Q4_K.pth"),     # exact width, the type is not offered at it: the first level of that width
    (4.5, None, "4.5-Q4_K.pth"),       # exact width, no type asked for
    (8.0, "Q8_0", "8.pth"),            # exact width of an untyped level
    (5.0, "Q6_K", "6.5625-Q6_K.pth"),  # no such width: the closest level OF THE PREFERRED TYPE, not the closest (4.5 / 5.5)
    (5.0, "Q3_K", "4.5-Q4_K.pth"),     # no such width, type not offered: the closest width, the first of two equally close
    (5.2, None, "5.5-Q5_0.pth"),       # no such width, no type: the closest width
    (1.0, "Q2_K", "2.5625-Q2_K.pth"),  # below every level
    (32.0, None, "8.pth"),             # above every level
])
def test_find_best_matching_config(width, qtype, want):
    from gptq_gguf_toolkit_amd.gguf_stitcher import GGUFStitcher
    assert GGUFStitcher._find_best_matching_config(None, LEVELS, width, qtype)["filename"] == want


def test_written_type_resolution():
    """An explicit type wins; otherwise the width class, the level's own quantization deciding inside a class."""
    from gptq_gguf_toolkit_amd.gguf_stitcher import GGUFStitcher, QuantizationConfig as Q
    f = lambda bw, t=None, orig="": GGUFStitcher._get_quantization_type_from_config(None, Q(bw, "x.pth", t), orig)  # noqa: E731
    assert [f(6.0, "Q2_K"), f(32), f(16), f(2), f(2.5625), f(2.0625), f(3.4375), f(3.44), f(4), f(4.5, None, "Q4_0"), f(4.25)] == \
        ["Q2_K", "F32", "F16", "Q2_K", "Q2_K", "IQ2_XXS", "Q3_K", "IQ3_S", "Q4_K", "Q4_0", "IQ4_XS"]
    assert [f(5.5), f(6.0), f(6.5625), f(8, None, "Q8_0"), f(8.5), f(1.5625), f(12), f(4.5, "NOPE")] == \
        ["Q5_K", "Q5_K", "Q6_K", "Q8_0", "Q8_K", "IQ1_S", "Q4_K", "Q4_K"]


# ------------------------------------------------------------------------------------------------ 4: general.file_type
def config_of(q2, q4, q6):
    """A configuration putting the first q2 projections on Q2_K, the next q4 on Q4_K, the next q6 on Q6_K (14 in all)."""
    names = [f"blk.{b}.{p}.weight" for b in range(2) for p, _, _ in PROJ]
    levels = [Q2_K] * q2 + [Q4_K] * q4 + [Q6_K] * q6
    return "".join(f"{n}: {EXACT[t].split('-')[0]} ({EXACT[t]}.pth)\n" for n, t in zip(names, levels))


# 21 tensors: the 14 projections, five F32 norms (width 32), token_embd (16) and output (Q6_K, 6.5625)
@pytest.mark.parametrize("counts,reference,llama", [
    ((0, 14, 0), 12, 15),   # 14 / 21 on 4.5: int(4.5) = 4 -> the ggml TYPE id of Q4_K (llama.cpp would read Q3_K_M)
    ((0, 0, 14), 14, 18),   # 15 / 21 on 6.5625 -> 14, where LLAMA_FTYPE_MOSTLY_Q6_K is 18
    ((5, 5, 4), 12, 15),    # no majority (5 / 5 / 5 / 5 / 1): 12, and MOSTLY_Q4_K_M for --llama-ftype
    ((8, 0, 6), 12, 15),    # no majority again (8 Q2_K, 6 + 1 Q6_K, 5 F32, 1 F16)
    ((7, 1, 6), 12, 15),    # a tie: 7 Q2_K and 6 + 1 Q6_K tensors; the first-seen width (2.5625) leads, without a majority
])
def test_file_type(world, tmp_path, counts, reference, llama):
    (tmp_path / "c.txt").write_text(config_of(*counts))
    for flag, want in ((False, reference), (True, llama)):
        out = tmp_path / f"{flag}.gguf"
        st = stitcher(world["mdb"], out, config=str(tmp_path / "c.txt"), llama_ftype=flag)
        assert st._calculate_file_type() == want
        st.stitch_model()
        kv, types, _ = read_kv(str(out))
        assert kv["general.file_type"] == want and types["general.file_type"] == 4


def test_file_type_tie_goes_to_the_first_width(world, tmp_path):
    """Two tensors on two widths: max() keeps the first-seen one (8.5 -> 7 in the reference's table if it had a majority);
    at exactly one half there is none, so 12 either way round.  --llama-ftype counts the planned tensors, not this
    hand-made configuration: its tie is the (7, 1, 6) case of test_file_type."""
    from gptq_gguf_toolkit_amd.gguf_stitcher import QuantizationConfig as Q
    st = stitcher(world["mdb"], tmp_path / "x.gguf")
    a, b = Q(8.5, "8.5-Q8_0.pth", "Q8_0"), Q(2.5625, "2.5625-Q2_K.pth", "Q2_K")
    for order in ((a, b), (b, a)):
        st.config = {"t0": order[0], "t1": order[1]}
        assert st._calculate_file_type() == 12
    st.config = {"t0": a, "t1": b, "t2": Q(8.5, "8.5-Q8_0.pth", "Q8_0")}
    assert st._calculate_file_type() == 7  # int(8.5) = 8 with two of three tensors


# ------------------------------------------------------------------------------------------------ 5: refusals
def add_iq_tensor(db):
    d = db / "blk.9.extra.weight"
    d.mkdir()
    (d / "2.06-IQ2_XXS.pth").write_bytes(bytes(66))
    (d / "2.06-IQ2_XXS-metadata.json").write_text(json.dumps({"tensor_info": {
        "name": d.name, "type": 16, "quantization": "IQ2_XXS", "shape": [256, 1], "np_dtype": "uint8", "np_shape": [1, 66]}}))


def break_missing(db, tmp):
    (tmp / "c.txt").write_text("blk.0.attn_q.weight: 3.4375 (3.4375-Q3_K.pth)\n")
    return "blk.0.attn_q.weight", "3.4375-Q3_K.pth"


def break_short(db, tmp):
    f = db / "blk.1.ffn_down.weight" / "4.5-Q4_K.pth"
    f.write_bytes(f.read_bytes()[:-1])
    return "blk.1.ffn_down.weight", "4.5-Q4_K.pth"


def break_type(db, tmp):
    add_iq_tensor(db)
    return "blk.9.extra.weight", "IQ2_XXS"


@pytest.mark.parametrize("breaker", [break_missing, break_short, break_type])
def test_refusals_leave_nothing_behind(world, tmp_path, capsys, breaker):
    from gptq_gguf_toolkit_amd import gguf_stitcher
    db, out = tmp_path / "db", tmp_path / "out.gguf"
    shutil.copytree(world["mdb"], db)
    (tmp_path / "c.txt").write_text("")
    tensor, word = breaker(db, tmp_path)
    st = stitcher(db, out, config=str(tmp_path / "c.txt"))
    with pytest.raises(gguf_stitcher.StitchError) as e:
        st.stitch_model()
    assert tensor in str(e.value) and word in str(e.value) and "1 tensors cannot be stitched" in str(e.value)
    assert not out.exists() and not (tmp_path / "out.gguf.partial").exists()
    # --validate-only reports the same problem, writes nothing and fails; so does the plain command
    for extra in (["--validate-only"], []):
        capsys.readouterr()
        assert gguf_stitcher.main([str(db), str(out), "--config", str(tmp_path / "c.txt")] + extra) == 1
        text = capsys.readouterr().out
        assert tensor in text and word in text
        assert not out.exists() and not (tmp_path / "out.gguf.partial").exists()


def test_fallback_to_the_f32_level(world, tmp_path):
    """A configured level that is not there falls back to the directory's 32-F32.pth, written as F32 (reference :592-598)."""
    (tmp_path / "c.txt").write_text("blk.0.attn_norm.weight: 4.5 (4.5-Q4_K.pth)\n")
    st = stitcher(world["mdb"], tmp_path / "o.gguf", config=str(tmp_path / "c.txt"))
    assert st.validate_config()
    st.stitch_model()
    got = {n: (gt, raw) for n, _, gt, raw in read_tensors(str(tmp_path / "o.gguf"))}
    assert got["blk.0.attn_norm.weight"] == (F32, (world["mdb"] / "blk.0.attn_norm.weight" / "32-F32.pth").read_bytes())


def test_a_failing_producer_leaves_nothing_behind(world, tmp_path, monkeypatch):
    from gptq_gguf_toolkit_amd.gguf_stitcher import GGUFStitcher
    out = tmp_path / "out.gguf"
    st = stitcher(world["mdb"], out)
    real, calls = GGUFStitcher._read_payload, []

    def failing(self, planned):
        calls.append(planned.name)
        if len(calls) == 3:
            raise OSError("injected: the third tensor cannot be read")
        return real(self, planned)

    monkeypatch.setattr(GGUFStitcher, "_read_payload", failing)
    with pytest.raises(OSError, match="injected"):
        st.stitch_model()
    assert len(calls) >= 3 and not out.exists() and not (tmp_path / "out.gguf.partial").exists()
    # an output from an earlier run is not touched by a failing one
    out.write_bytes(b"earlier")
    calls.clear()
    with pytest.raises(OSError, match="injected"):
        stitcher(world["mdb"], out).stitch_model()
    assert out.read_bytes() == b"earlier" and not (tmp_path / "out.gguf.partial").exists()


def test_key_value_source_is_checked_before_anything_is_written(world, tmp_path, capsys):
    """An alignment other than the writer's 32 would contradict the file's layout, and a source without key/value data
    would give a file llama.cpp cannot load: both are refused with the tensors, by the library and by both commands."""
    from gptq_gguf_toolkit_amd import gguf_stitcher
    out = tmp_path / "out.gguf"
    for word, change in (("general.alignment is 64", lambda md: md["general.alignment"].update(value=64)),
                         ("no key/value data", lambda md: md.clear())):
        db = tmp_path / word.split()[0]
        shutil.copytree(world["udb"], db)
        man = json.loads((db / "manifest.json").read_text())
        change(man["metadata"])
        man["model_info"]["original_file"] = "gone.gguf"
        (db / "manifest.json").write_text(json.dumps(man))
        with pytest.raises(gguf_stitcher.StitchError, match=word) as e:
            stitcher(db, out).stitch_model()
        assert "0 tensors cannot be stitched" in str(e.value)
        for extra in (["--validate-only"], []):
            capsys.readouterr()
            assert gguf_stitcher.main([str(db), str(out)] + extra) == 1
            assert word in capsys.readouterr().out
        assert not out.exists() and not (tmp_path / "out.gguf.partial").exists()
        assert gguf_stitcher.main([str(db), str(out), "--original-model", world["uniform"]]) == 0  # the original's keys are fine
        out.unlink()


def test_every_tensor_is_resolved_once_per_run(world, tmp_path, monkeypatch):
    """validate_config, stitch_model and the --llama-ftype count share one plan."""
    from gptq_gguf_toolkit_amd import gguf_stitcher
    real, calls = gguf_stitcher.GGUFStitcher._resolve, []
    monkeypatch.setattr(gguf_stitcher.GGUFStitcher, "_resolve", lambda self, n, c: calls.append(n) or real(self, n, c))
    assert gguf_stitcher.main([str(world["mdb"]), str(tmp_path / "o.gguf"), "--llama-ftype"]) == 0
    assert len(calls) == 21 == len(set(calls))


def test_quiet_leaves_out_the_line_per_tensor(world, tmp_path, capsys):
    capsys.readouterr()
    stitcher(world["mdb"], tmp_path / "o.gguf")
    assert "blk.0.attn_q.weight: Using" in capsys.readouterr().out
    stitcher(world["mdb"], tmp_path / "o.gguf", quiet=True)
    text = capsys.readouterr().out
    assert ": Using" not in text and "Total configuration: 21 tensors" in text


# ------------------------------------------------------------------------------------------------ 6: streaming
def test_payloads_are_read_while_the_file_is_written(world, tmp_path, monkeypatch):
    """Structural: when the writer hands its FIRST payload to the file, fewer level files have been read than there are
    tensors -- the pipeline depth of GGUFWriter bounds the read-ahead, not the model."""
    import builtins
    from gptq_gguf_toolkit_amd import gguf_writer
    from gptq_gguf_toolkit_amd.gguf_stitcher import GGUFStitcher
    real, produced, at_first_payload = GGUFStitcher._read_payload, [], []

    def counting(self, planned):
        produced.append(planned.name)
        return real(self, planned)

    class Spy:
        def __init__(self, f):
            self.f = f

        def write(self, b):
            if isinstance(b, memoryview) and not at_first_payload:  # payloads are written from the arrays' own buffers
                at_first_payload.append(len(produced))
            return self.f.write(b)

        def __getattr__(self, name):
            return getattr(self.f, name)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            self.f.close()

    monkeypatch.setattr(GGUFStitcher, "_read_payload", counting)
    monkeypatch.setattr(gguf_writer, "open", lambda *a, **k: Spy(builtins.open(*a, **k)), raising=False)
    st = stitcher(world["mdb"], tmp_path / "o.gguf")
    assert produced == []  # nothing is read before the file is written
    st.stitch_model()
    bound = gguf_writer.GGUFWriter.LAZY_DEPTH + 2 * gguf_writer.GGUFWriter.LAZY_WORKERS
    assert len(produced) == 21 and 1 <= at_first_payload[0] <= bound < 21
    assert read_tensors(str(tmp_path / "o.gguf"))[20][0] == "output.weight"


# ------------------------------------------------------------------------------------------------ reports, both-sided db
def test_reports(world, tmp_path, capsys):
    from gptq_gguf_toolkit_amd import gguf_stitcher
    capsys.readouterr()
    assert gguf_stitcher.main([str(world["mdb"]), str(tmp_path / "o.gguf"), "--list-tensors"]) == 0
    text = capsys.readouterr().out
    assert "blk.0.attn_q.weight:\n  - 2.5625-bit (Q2_K) [2.5625-Q2_K.pth]\n  - 4.5-bit (Q4_K) [4.5-Q4_K.pth]\n  - 6.5625-bit (Q6_K)" in text
    assert gguf_stitcher.main([str(world["mdb"]), str(tmp_path / "o.gguf"), "--inspect-metadata", "--original-model",
                               world["levels"][Q4_K]]) == 0
    text = capsys.readouterr().out
    assert "llama.block_count: 2 (type: UINT32)" in text and "Manifest metadata: 14 keys" in text
    assert not (tmp_path / "o.gguf").exists()


def test_database_split_on_both_sides(world, tmp_path):
    """`gguf_splitter --both` leaves the HF side's manifest as manifest.json and its directories of torch-saved tensors next
    to the GGUF ones: those are not GGUF tensors, and the file's tensor order comes from gguf_layer_database.json."""
    db = tmp_path / "db"
    shutil.copytree(world["udb"], db)
    layers = {}
    for b in range(2):
        d = db / f"model.layers.{b}.self_attn.q_proj"
        d.mkdir()
        (d / "4.5-Q4_K.pth").write_bytes(b"a torch pickle")
        layers[f"model.layers.{b}.self_attn.q_proj.weight"] = {"layer_directory": d.name, "filename": "4.5-Q4_K.pth"}
    (db / "manifest.json").write_text(json.dumps({"model_info": {"original_file": "uniform.gguf"}, "layers": layers}))
    st = stitcher(db, tmp_path / "o.gguf", original_model_path=world["uniform"])
    st.stitch_model()
    want, got = read_tensors(world["uniform"]), read_tensors(str(tmp_path / "o.gguf"))
    assert got == want
    assert read_kv(str(tmp_path / "o.gguf"))[0]["llama.some_uint64"] == 2 ** 40
    # that manifest has no key/value data: without the original there is nothing to write, and nothing is written
    from gptq_gguf_toolkit_amd.gguf_stitcher import StitchError
    with pytest.raises(StitchError, match="no key/value data"):
        stitcher(db, tmp_path / "none.gguf").stitch_model()
    assert not (tmp_path / "none.gguf").exists() and not (tmp_path / "none.gguf.partial").exists()
