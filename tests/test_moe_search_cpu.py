"""K30, host side (no GPU): the gq_level_switch_experts symbol and every one of its refusals, level_db on the 3-D sidecars of
stacked expert tensors, LevelStore's expert units (its refusals by name, and its bookkeeping with the two switch calls replaced
by torch copies on CPU tensors), and the search's host logic -- bit accounting, grouping, the configuration text -- on units."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")

E, H, I = 3, 256, 512
MOD = "model.layers.0.mlp.experts"
UNITS = [f"{MOD}.{r}_proj" for r in ("gate", "up", "down")]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbol_is_declared_exported_and_bound():
    from gptq_gguf_toolkit_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "gptq_gguf_moe_search.h")).read()
    declared = set(re.findall(r"\b(gq_[a-z0-9_]+)\s*\(", hdr))
    L = _cabi.lib()
    assert declared == set(_cabi.EXPORTS_MOE_SEARCH) == {"gq_level_switch_experts"}
    assert len(_cabi.EXPORTS) == 48 and not declared & set(_cabi.EXPORTS)
    assert hasattr(ctypes.CDLL(_cabi.SO_PATH), "gq_level_switch_experts") and L.gq_level_switch_experts.argtypes
    assert L.gq_abi_version() == _cabi.ABI_VERSION == 6  # additive: the version stays
    m = re.search(r"#define GQ_SWITCH_EXPERTS_MAX_JOBS (\d+)", hdr)
    assert m and int(m.group(1)) == _cabi.SWITCH_EXPERTS_MAX_JOBS
    # the C struct and its ctypes image: 2 pointers, 4 int64, 2 int32
    J = _cabi.SwitchExpertsJob
    assert ctypes.sizeof(J) == 56 and J.dst_expert_stride.offset == 40 and J.kind.offset == 48 and J.out_dtype.offset == 52
    # the table of MAX_JOBS entries of 56 bytes (and 8 of header) is the largest that fits what gq_level_switch allows itself
    assert 8 + 56 * int(m.group(1)) <= 4096 - 64 < 8 + 56 * (int(m.group(1)) + 1)
    src = open(os.path.join(ROOT, "gptq-gguf-toolkit_amd", "csrc", "search", "gq_switch_experts.hip")).read()
    assert "static_assert(sizeof(ExpertsTable) <= TABLE_ROOM" in src


def test_every_refusal_needs_no_device():
    """Every check comes before the first HIP call: a negative status and a message naming the job and the argument, on a
    machine without a GPU and with pointers that are never dereferenced."""
    from gptq_gguf_toolkit_amd import _cabi
    L, J = _cabi.lib(), _cabi.SwitchExpertsJob
    p = 4096  # any 16-byte aligned address

    def refused(jobs, status, *words):
        rc = L.gq_level_switch_experts((J * len(jobs))(*jobs), len(jobs), None)
        msg = L.gq_last_error().decode()
        assert rc == status and "gq_level_switch_experts" in msg and all(w in msg for w in words), (rc, msg)

    def job(src=p, dst=p, E=4, R=4, C=256, stride=None, kind=12, out=1):
        return J(src, dst, E, R, C, R * C if stride is None else stride, kind, out)

    ok = job()
    assert L.gq_level_switch_experts(None, 0, None) == 0  # n_jobs = 0: a no-op, the table is not read
    assert L.gq_level_switch_experts((J * 1)(ok), 0, None) == 0
    assert L.gq_level_switch_experts((J * 1)(ok), -1, None) == -2 and "n_jobs" in L.gq_last_error().decode()
    assert L.gq_level_switch_experts(None, 1, None) == -6 and "jobs_host" in L.gq_last_error().decode()
    refused([job(src=None)], -6, "job 0", "src is NULL")
    refused([ok, job(dst=None)], -6, "job 1", "dst is NULL")
    for kind in (9, 15, 3, 24):
        refused([ok, ok, job(kind=kind)], -1, "job 2", f"kind {kind}")
    refused([job(out=3)], -1, "job 0", "out_dtype 3")
    refused([job(E=0)], -2, "job 0", "E=0")
    refused([job(E=-1)], -2, "job 0", "E=-1")
    refused([job(E=65536)], -2, "job 0", "E=65536")
    refused([job(R=0)], -2, "job 0", "R=0")
    refused([job(C=0)], -2, "job 0", "C=0")
    refused([job(C=384)], -2, "job 0", "C=384")                     # K-quants: C % 256
    refused([job(C=384, kind=23)], -2, "job 0", "C=384")            # IQ4_XS: C % 256
    refused([job(C=48, kind=8)], -2, "job 0", "C=48")               # Q8_0: C % 32
    refused([job(C=48, kind=20)], -2, "job 0", "C=48")              # IQ4_NL: C % 32
    refused([job(C=260, kind=1, out=2)], -2, "job 0", "C=260")      # dense: fp16 rows of 520 bytes
    refused([job(C=252, kind=0, out=1)], -2, "job 0", "C=252")      # fp32 rows fit, fp16 rows of 504 bytes do not
    refused([job(stride=4 * 256 - 8)], -2, "job 0", "dst_expert_stride=1016")       # < R * C
    refused([job(stride=4 * 256 + 4)], -2, "job 0", "dst_expert_stride=1028", "16 bytes")  # fp16: 2056 bytes
    refused([job(stride=4 * 256 + 2, out=0)], -2, "job 0", "dst_expert_stride=1026", "16 bytes")  # fp32: 4104 bytes
    refused([job(dst=p + 8)], -2, "job 0", "dst not 16-byte aligned")
    refused([job(src=p + 8)], -2, "job 0", "src not 16-byte aligned")             # Q4_K: 16
    refused([job(src=p + 8, kind=13)], -2, "job 0", "src not 16-byte aligned")    # Q5_K: 16
    refused([job(src=p + 4, kind=23)], -2, "job 0", "src not 8-byte aligned")     # IQ4_XS: 8
    refused([job(src=p + 2, kind=10)], -2, "job 0", "src not 4-byte aligned")     # Q2_K: 4
    refused([job(src=p + 1, kind=11)], -2, "job 0", "src not 2-byte aligned")     # Q3_K: 2
    refused([job(src=p + 3, kind=14)], -2, "job 0", "src not 2-byte aligned")     # Q6_K
    refused([job(src=p + 1, kind=8, C=32)], -2, "job 0", "src not 2-byte aligned")    # Q8_0
    refused([job(src=p + 4, kind=1, out=2)], -2, "job 0", "src not 16-byte aligned")  # dense
    refused([job(R=1 << 50)], -2, "job 0", "more than one launch")
    refused([job(E=65535, R=1 << 20, C=4096)], -2, "job 0", "E=65535", "more than one launch")
    # the refusal of a late job comes before any launch of the earlier ones: more jobs than one launch takes, the last one bad
    n = _cabi.SWITCH_EXPERTS_MAX_JOBS + 2
    refused([ok] * (n - 1) + [job(dst=None)], -6, f"job {n - 1}", "dst is NULL")
    # (an expert's slice keeps the type's alignment whenever src does -- every block size is a multiple of its alignment --, so
    # Q3_K with an odd number of blocks per expert is taken: tests/test_gpu_moe_search.py runs it, 21 blocks of 110 bytes)


def test_ops_binding_checks_its_views():
    from gptq_gguf_toolkit_amd import _cabi, ops
    assert ops.level_switch_experts([]) is None and ops.SWITCH_EXPERTS_MAX_JOBS == _cabi.SWITCH_EXPERTS_MAX_JOBS
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.level_switch_experts([(torch.zeros(2, 4, 256), torch.zeros(2, 4, 256, dtype=torch.float16), None)])


# ------------------------------------------------------------------------------------------------ level_db on 3-D sidecars
def _expert_db(path, dtype=np.float16, levels=(("F16", 1), ("F32", 0))):
    """A database of the three stacked tensors of block 0 (and a 2-D attn_q) with plain levels, written by LevelDbWriter (the
    sidecars are level_records', the splitter's)."""
    from gptq_gguf_toolkit_amd import level_db
    rng = np.random.default_rng(0)
    want = {}
    with level_db.LevelDbWriter(path) as w:
        for role, shape in (("gate", (E, I, H)), ("up", (E, I, H)), ("down", (E, H, I))):
            for name, gt in levels:
                a = rng.standard_normal(shape).astype(np.float16 if gt == 1 else np.float32)
                w.add_level(f"blk.0.ffn_{role}_exps.weight", shape, gt, a)
                want[f"{MOD}.{role}_proj", name] = torch.from_numpy(a)
        w.add_level("blk.0.attn_q.weight", (H, H), 1, rng.standard_normal((H, H)).astype(np.float16))
    return want


def test_level_db_reads_3d_sidecars_and_finds_the_unit_directories(tmp_path):
    from gptq_gguf_toolkit_amd import level_db
    db = str(tmp_path / "db")
    _expert_db(db)
    for role in ("gate", "up", "down"):
        d = level_db.layer_dir(db, f"{MOD}.{role}_proj")
        assert d == os.path.join(db, f"blk.0.ffn_{role}_exps.weight") and level_db.has_layer(db, f"{MOD}.{role}_proj")
        assert level_db.level_files(d) == ["16-F16.pth", "32-F32.pth"]
        rec = level_db.read_sidecar(os.path.join(d, "16-F16.pth"))
        shape = (E, H, I) if role == "down" else (E, I, H)
        assert rec.shape == shape and rec.np_shape == list(shape) and rec.ggml_type == 1
        assert level_db.check_level_size(rec) == 2 * E * H * I == rec.nbytes
    assert level_db.expert_unit(f"{MOD}.gate_proj") == (MOD, "gate")
    assert level_db.expert_unit("model.layers.0.mlp.gate_proj") is None  # a dense model's Linear keeps its own rule
    assert level_db.expert_unit_tensor("model.layers.7.mlp.experts.down_proj") == "blk.7.ffn_down_exps.weight"
    assert not level_db.has_layer(db, "model.layers.1.mlp.experts.gate_proj") and not level_db.has_layer(db, f"{MOD}.w1")
    assert level_db.layer_dir(db, "model.layers.0.self_attn.q_proj") == os.path.join(db, "blk.0.attn_q.weight")
    # a packed 3-D level: np_shape is [E, R, row bytes]
    side, _, _ = level_db.level_records("blk.0.ffn_gate_exps.weight", (E, I, H), 12, "Q4_K", 4.5, 4.5, E * I * 144, "4.5-Q4_K")
    assert side["np_shape"] == [E, I, 144] and side["shape"] == [H, I, E] and side["n_elements"] == E * I * H
    # a file shorter than its sidecar describes is refused
    f = os.path.join(db, "blk.0.ffn_up_exps.weight", "16-F16.pth")
    with open(f, "r+b") as fh:
        fh.truncate(2 * E * H * I - 2)
    with pytest.raises(ValueError, match=rf"np_shape \[{E}, {I}, {H}\]"):
        level_db.check_level_size(level_db.read_sidecar(f))


def test_a_dense_tensors_records_are_what_they_were():
    """The 2-D side of level_records, byte for byte the JSON the splitter has always written."""
    from gptq_gguf_toolkit_amd import level_db
    side, level, rec = level_db.level_records("blk.0.attn_q.weight", (256, 512), 12, "Q4_K", 4.5, 4.5, 256 * 2 * 144, "4.5-Q4_K", 96)
    assert json.dumps(side) == json.dumps({
        "name": "blk.0.attn_q.weight", "type": 12, "quantization": "Q4_K", "bitwidth": 4.5, "exact_bitwidth": 4.5,
        "shape": [512, 256], "n_elements": 131072, "n_bytes": 73728, "data_offset_original": 96,
        "data_filename": "4.5-Q4_K.pth", "np_dtype": "uint8", "np_shape": [256, 288]})
    assert rec == {"tensor_type": 12, "quantization": "Q4_K", "bitwidth": 4.5, "exact_bitwidth": 4.5, "shape": [512, 256],
                   "n_elements": 131072, "n_bytes": 73728, "data_offset": 96}
    assert level["filename"] == "4.5-Q4_K.pth" and level["size_bytes"] == 73728


# ------------------------------------------------------------------------------------------------ LevelStore
class Experts(torch.nn.Module):
    """The parameters of transformers' MixtralExperts, nothing else."""

    def __init__(self, dtype=torch.float16):
        super().__init__()
        self.gate_up_proj = torch.nn.Parameter(torch.full((E, 2 * I, H), -7.0, dtype=dtype))
        self.down_proj = torch.nn.Parameter(torch.full((E, H, I), -7.0, dtype=dtype))
        self.act_fn = torch.nn.SiLU()


def _model(experts=None):
    m = torch.nn.Module()
    m.model = torch.nn.Module()
    m.model.layers = torch.nn.ModuleList([torch.nn.Module()])
    m.model.layers[0].mlp = torch.nn.Module()
    m.model.layers[0].mlp.experts = Experts() if experts is None else experts
    m.model.layers[0].self_attn = torch.nn.Module()
    m.model.layers[0].self_attn.q_proj = torch.nn.Linear(H, H, bias=False).half()
    return m


def test_level_store_refuses_what_is_no_unit_by_name(tmp_path):
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    db = str(tmp_path / "nothing-is-read")
    per_expert = torch.nn.ModuleList([torch.nn.Module() for _ in range(2)])
    for e in per_expert:
        e.w1, e.w2, e.w3 = (torch.nn.Linear(8, 8, bias=False) for _ in range(3))
    with pytest.raises(TypeError, match=r"model\.layers\.0\.mlp\.experts\.gate_proj.*per-expert w1 / w2 / w3"):
        LevelStore(_model(per_expert), db, "cpu", [f"{MOD}.gate_proj"])
    odd = Experts()
    odd.down_proj = torch.nn.Parameter(torch.zeros(E, H, I + 1))
    with pytest.raises(TypeError, match=r"model\.layers\.0\.mlp\.experts\.up_proj.*without gate_up_proj"):
        LevelStore(_model(odd), db, "cpu", [f"{MOD}.up_proj"])
    with pytest.raises(TypeError, match=r"model\.layers\.0\.mlp\.experts is a Experts"):
        LevelStore(_model(), db, "cpu", [MOD])                      # the module itself is no layer: name its units
    with pytest.raises(TypeError, match=r"model\.layers\.0\.mlp\.nothing\.gate_proj.*does not exist"):
        LevelStore(_model(), db, "cpu", ["model.layers.0.mlp.nothing.gate_proj"])
    with pytest.raises(TypeError, match=r"neither a module of the model nor an expert unit"):
        LevelStore(_model(), db, "cpu", [f"{MOD}.w1"])
    assert not os.path.exists(db)


def test_level_store_units_with_the_switch_calls_replaced_by_copies(tmp_path, monkeypatch):
    """Dense residency on CPU tensors: default discovery, the shape check, one stacked job per changed unit into the unit's
    slice of the fused parameter (the other slices and both data_ptr()s untouched), jobs_issued counting units."""
    from gptq_gguf_toolkit_amd import level_store as LS
    db = str(tmp_path / "db")
    want = _expert_db(db)
    calls = []

    def fake_experts(jobs):
        calls.append(len(jobs))
        for src, dst, kind in jobs:
            assert kind is None and dst.dim() == 3 and dst[0].is_contiguous() and tuple(src.shape) == tuple(dst.shape)
            dst.copy_(src.to(dst.dtype))

    def fake_linear(jobs):
        for src, dst, kind, rows in jobs:
            dst.copy_(src.to(dst.dtype))

    monkeypatch.setattr(LS.ops, "level_switch_experts", fake_experts)
    monkeypatch.setattr(LS.ops, "level_switch", fake_linear)
    monkeypatch.setattr(LS.level_db, "rotary_rows", lambda *a: None)
    m = _model()
    ex = m.model.layers[0].mlp.experts
    store = LS.LevelStore(m, db, "cpu")
    assert list(store.layers) == UNITS + ["model.layers.0.self_attn.q_proj"]
    assert store.units == {u: (MOD, u.rsplit(".", 1)[1][:-5]) for u in UNITS}
    assert store.shape_of(UNITS[0]) == (E, I, H) and store.shape_of(UNITS[2]) == (E, H, I)
    assert all(store.level_keys(u) == [16.0, 32.0] for u in UNITS)
    ptrs = (ex.gate_up_proj.data_ptr(), ex.down_proj.data_ptr())
    assert store.switch({UNITS[1]: 16.0}) == 1 and store.jobs_issued == 1 and calls == [1]
    assert torch.equal(ex.gate_up_proj.data[:, I:], want[UNITS[1], "F16"])
    assert bool((ex.gate_up_proj.data[:, :I] == -7).all()) and bool((ex.down_proj.data == -7).all())  # the gate half: untouched
    assert store.switch({u: 32.0 for u in UNITS}) == 3 and store.jobs_issued == 4 and calls == [1, 3]
    assert torch.equal(ex.gate_up_proj.data[:, :I], want[UNITS[0], "F32"].half())
    assert torch.equal(ex.gate_up_proj.data[:, I:], want[UNITS[1], "F32"].half())
    assert torch.equal(ex.down_proj.data, want[UNITS[2], "F32"].half())
    assert store.switch({u: 32.0 for u in UNITS}) == 0 and store.jobs_issued == 4  # nothing changed: no job
    assert (ex.gate_up_proj.data_ptr(), ex.down_proj.data_ptr()) == ptrs
    got = store.weight_of(UNITS[2], 16.0)
    assert tuple(got.shape) == (E, H, I) and torch.equal(got, want[UNITS[2], "F16"])
    assert store.level_tensor(UNITS[0], 32.0).dtype == torch.float32 and tuple(store.level_tensor(UNITS[0], 32.0).shape) == (E, I, H)
    # a module of another shape is refused by the unit's name, before any upload
    other = Experts()
    other.gate_up_proj = torch.nn.Parameter(torch.zeros(E, 2 * H, I, dtype=torch.float16))
    other.down_proj = torch.nn.Parameter(torch.zeros(E, I, H, dtype=torch.float16))
    with pytest.raises(ValueError, match=r"experts\.gate_proj: level '16-F16.pth' has shape \(3, 512, 256\), the expert unit \(3, 256, 512\)"):
        LS.LevelStore(_model(other), db, "cpu", UNITS)


def test_level_store_packed_residency_installs_packed_experts(tmp_path, monkeypatch):
    """Packed residency: the module becomes a PackedExperts once, its dense bytes are freed and credited once, a switch is
    set_level without a launch, and a module held in part is refused."""
    from gptq_gguf_toolkit_amd import level_store as LS
    from gptq_gguf_toolkit_amd.packed_experts import PackedExperts
    db = str(tmp_path / "db")
    want = _expert_db(db, levels=(("F16", 1),))
    monkeypatch.setattr(LS.ops, "level_switch_experts", lambda jobs: pytest.fail("packed residency launches nothing"))
    with pytest.raises(ValueError, match=r"needs all three expert units.*up_proj"):
        LS.LevelStore(_model(), db, "cpu", [UNITS[0], UNITS[2]], resident="packed")
    m = _model()
    dense = 2 * (E * 2 * I * H + E * H * I)
    store = LS.LevelStore(m, db, "cpu", UNITS, resident="packed", moe_prefill="grouped")
    px = m.model.layers[0].mlp.experts
    assert isinstance(px, PackedExperts) and px.prefill == "grouped" and store.freed_bytes == dense
    assert all(store.layers[u] is px for u in UNITS) and store.shape_of(UNITS[2]) == (E, H, I)
    assert store.switch({u: 16.0 for u in UNITS}) == 3 and store.jobs_issued == 0
    for u, role in zip(UNITS, ("gate", "up", "down")):
        blocks, kind = px.levels[role]
        assert kind is None and blocks is store.find(u, 16.0).data and torch.equal(blocks, want[u, "F16"])
    assert LS.packed_peak_bytes([10, 10, 10], [dense, 0, 0]) == 30 - dense  # the module's bytes are credited at its first unit


# ------------------------------------------------------------------------------------------------ the search's host logic
class FakeMoE:
    """get_submodule() of a 2-block fused-experts model: Linears with weight.numel(), experts modules with down_proj.shape."""
    ATT = {"self_attn.q_proj": H * H, "self_attn.k_proj": H * H // 2, "self_attn.v_proj": H * H // 2, "self_attn.o_proj": H * H}

    def get_submodule(self, name):
        if name.endswith(".mlp.experts"):
            return types.SimpleNamespace(down_proj=types.SimpleNamespace(shape=(E, H, I)))
        n = self.ATT[name.split(".", 3)[3]]
        return types.SimpleNamespace(weight=types.SimpleNamespace(numel=lambda: n))


def test_search_counts_groups_and_names_units():
    import random
    from gptq_gguf_toolkit_amd import config_converter, evo_quant_search as S
    model = FakeMoE()
    names = [f"model.layers.{b}.{k}" for b in range(2) for k in list(FakeMoE.ATT) + [f"mlp.experts.{r}_proj" for r in ("gate", "up", "down")]]
    names = sorted(names, key=S.layer_order_fn)
    units = [n for n in names if ".experts." in n]
    assert all(S.layer_numel(model, u) == E * H * I for u in units)
    assert S.layer_numel(model, "model.layers.1.self_attn.k_proj") == H * H // 2
    by_size = S.group_layers(model, names, "size")
    assert sorted(map(sorted, by_size)) == sorted(map(sorted, [
        units, [n for n in names if n.endswith(("q_proj", "o_proj"))], [n for n in names if n.endswith(("k_proj", "v_proj"))]]))
    assert any({f"model.layers.0.mlp.experts.gate_proj", "model.layers.0.mlp.experts.up_proj"} <= set(g) for g in by_size)
    by_name = S.group_layers(model, names, "name")
    assert ["model.layers.0.mlp.experts.gate_proj", "model.layers.1.mlp.experts.gate_proj"] in [list(g) for g in by_name]
    state = [[4.5] * len(g) for g in by_size]
    per_block = 3 * E * H * I + 3 * H * H
    assert S.calculate_total_bits(state, by_size, model) == 2 * per_block * 4.5
    assert S.target_bits_of(by_size, model, 4.5) == int(2 * per_block * 4.5)
    bws = [(2.5625, "2.5625-Q2_K.pth"), (4.5, "4.5-Q4_K.pth"), (6.5625, "6.5625-Q6_K.pth")]
    levels = {n: list(bws) for n in names}
    ctx = S._Ctx(model, by_size, levels, S.target_bits_of(by_size, model, 4.5))
    g = next(i for i, grp in enumerate(by_size) if units[0] in grp)
    assert S.get_next_bitwidth(state, ctx.target_bits, by_size, levels, model, g, 0, "increase") is None  # E*H*I * 2.0625 too many
    lowered = [list(r) for r in state]
    lowered[g][1] = lowered[g][2] = 2.5625
    assert S.get_next_bitwidth(lowered, ctx.target_bits, by_size, levels, model, g, 0, "increase") == 6.5625
    child = S.mutate(state, random.Random(1), ctx, "size")
    assert child is None or ctx.bits(child) <= ctx.target_bits
    text = S.configuration_text(by_size, lowered, levels)
    assert by_size[g][1] in units and f"{by_size[g][1]}: 2.5625 (2.5625-Q2_K.pth)" in text.split("\n")
    assert all(f"{u}: " in text for u in units)
    # the text goes through config_converter to the stacked tensors' names
    assert config_converter.detect_moe_model(text)
    gg = config_converter.convert_hf_to_gguf_config(text, is_moe=True)
    for b in range(2):
        for r in ("gate", "up", "down"):
            assert gg[f"blk.{b}.ffn_{r}_exps.weight"].endswith(".pth)")
