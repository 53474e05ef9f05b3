"""IQ4_NL and IQ4_XS on the GPU: gq_dequantize_blocks and gq_level_switch against the scalar restatement of the two decoders
(tests/iq4_spec.py, bit for bit), the four packed-forward entry points against it, against fp64, against themselves and against
each other, and a small Llama written as a .gguf of the two types: loaded dense and packed, and switched by a LevelStore.
Fixtures and their properties are pinned on the host by tests/test_iq4_cpu.py; helpers are test_gpu_qgemm.py's."""
import copy
import re

import numpy as np
import pytest

import iq4_spec as S
from test_gpu_decode import bits
from test_gpu_qgemm import BF16, F16, FILL, guarded_y, guards_intact, ops, subnormal  # noqa: F401
from test_gpu_qgemm import raw_call as raw_linear
from test_gpu_qgemv import raw_call as raw_gemv

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NL, XS = S.NL, S.XS
F32 = torch.float32
IDS = lambda cases: [f"{S.NAME[c[0]]}-{c[1]}x{c[2]}" for c in cases]  # noqa: E731
_spec = {}


def spec(t, blocks, key):
    """The scalar decode of a fixture as a CPU fp32 tensor: computed once per key, never changed."""
    if key not in _spec:
        _spec[key] = torch.from_numpy(S.decode(t, blocks))
    return _spec[key]


def upload(blocks, offset=0):
    """The bytes on the device as a 1-D view that starts `offset` bytes after a 16-byte aligned address."""
    raw = torch.from_numpy(np.ascontiguousarray(blocks)).reshape(-1)
    buf = torch.zeros(offset + raw.numel() + 16, dtype=torch.uint8, device="cuda")
    src = buf[offset:offset + raw.numel()]
    src.copy_(raw)
    assert src.data_ptr() % 16 == offset
    return src


def permutation(R, seed):
    return torch.randperm(R, generator=torch.Generator().manual_seed(seed)).to(torch.int32)


# ------------------------------------------------------------------------------------------------ 1: gq_dequantize_blocks
@pytest.mark.parametrize("gather", [False, True], ids=["identity", "gathered"])
@pytest.mark.parametrize("t,R,C", S.DEQUANT_CASES, ids=IDS(S.DEQUANT_CASES))
def test_dequantize_blocks_is_the_spec_bit_for_bit(ops, t, R, C, gather):  # noqa: F811
    """All three output dtypes; the source at the type's own alignment (2 / 8 bytes past a 16-byte boundary); the output
    between two guard rows."""
    from gptq_gguf_toolkit_amd import _cabi
    from gptq_gguf_toolkit_amd.ops import _DT, _ptr, _stream
    blocks = S.dequant_fixture(t, R, C)
    want32 = spec(t, blocks, ("deq", t, R, C))
    assert bool(torch.isfinite(want32).all())
    rows = permutation(R, R + C) if gather else None
    if rows is not None:
        want32 = want32[rows.long()]
    src = upload(blocks, offset=2 if t == NL else 8)
    for dt in (F32, F16, BF16):
        want = want32.to(dt).cuda()  # (the fp32 value is finite; the cast to fp16 overflows to inf where torch's does)
        buf = torch.empty(R + 2, C, dtype=dt, device="cuda")
        bits(buf).fill_(0x5A5A)
        out = buf[1:R + 1]
        assert out.data_ptr() % 16 == 0
        rc = _cabi.lib().gq_dequantize_blocks(t, _ptr(src), R, C, _ptr(rows.cuda()) if gather else None, _ptr(out), _DT[dt],
                                              _stream(src))
        assert rc == 0, _cabi.lib().gq_last_error()
        assert torch.equal(bits(out), bits(want)), f"{dt}: {int((bits(out) != bits(want)).sum())} of {want.numel()} values differ"
        assert bool((bits(buf[0]) == 0x5A5A).all()) and bool((bits(buf[R + 1]) == 0x5A5A).all()), "written outside out"
        got = ops.dequantize_blocks(t, src.view(R, -1), dt, rows.cuda() if gather else None)  # the binding: the same call
        assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("t,R,C", [(XS, 5, 512), (NL, 5, 96)], ids=["IQ4_XS", "IQ4_NL"])
def test_a_non_finite_d_propagates(ops, t, R, C):  # noqa: F811
    blocks = S.with_inf_block(t, S.dequant_fixture(t, R, C))
    want32 = spec(t, blocks, ("inf", t, R, C))
    nan = torch.isnan(want32)
    bs = S.GEOMETRY[t][0]  # block 1 is non-finite throughout: NaN where ls == 32 (its first sub-block), inf elsewhere
    assert int((~torch.isfinite(want32)).sum()) == bs and (int(nan.sum()) >= 32 if t == XS else not bool(nan.any()))
    for dt in (F32, F16, BF16):
        got = ops.dequantize_blocks(t, upload(blocks).view(R, -1), dt).cpu()
        want = want32.to(dt)
        assert torch.equal(torch.isnan(got), nan)
        assert torch.equal(bits(got)[~nan], bits(want)[~nan])


# ------------------------------------------------------------------------------------------------ 2: gq_level_switch
def test_one_switch_launch_decodes_every_kind(ops):  # noqa: F811
    """Q4_K, IQ4_XS, IQ4_NL, Q8_0 and a dense job in one call: every destination is dequantize_blocks of its source."""
    g = torch.Generator().manual_seed(11)
    W4, W8, Wd = (torch.randn(5, 512, generator=g).cuda(), torch.randn(5, 96, generator=g).cuda(),
                  torch.randn(8, 64, generator=g).cuda())
    q4 = ops.pack(12, *ops.rtn_quantize(W4, 12))
    q8 = ops.quantize_q8_0(W8)
    xs, nl = upload(S.dequant_fixture(XS, 33, 768), 8), upload(S.dequant_fixture(NL, 67, 288), 2)
    rows = permutation(67, 5).cuda()
    jobs, want = [], []
    for src, kind, shape, dt, r in ((q4, 12, (5, 512), F16, None), (xs, XS, (33, 768), BF16, None), (nl, NL, (67, 288), F32, rows),
                                    (q8, 8, (5, 96), F16, None), (Wd, None, (8, 64), F16, None), (xs, XS, (33, 768), F16, None),
                                    (nl, NL, (67, 288), BF16, None)):
        dst = torch.empty(*shape, dtype=dt, device="cuda")
        bits(dst).fill_(0x5A5A)
        jobs.append((src, dst, kind, r))
        want.append(Wd.to(dt) if kind is None else ops.dequantize_blocks(kind, src.view(shape[0], -1), dt, r))
    ops.level_switch(jobs)
    for i, ((_, dst, kind, _), w) in enumerate(zip(jobs, want)):
        assert torch.equal(bits(dst), bits(w)), (i, kind)
    assert torch.equal(bits(jobs[1][1].cpu()), bits(spec(XS, S.dequant_fixture(XS, 33, 768), ("deq", XS, 33, 768)).to(BF16)))


# ------------------------------------------------------------------------------------------------ 3: the packed forward
def gemm_weight(t, R, C, gather):
    """(blocks on the device at the type's own alignment, row_src or None, the spec's weight fp32 on the CPU, rows applied)."""
    blocks = S.gemm_fixture(t, R, C)
    want = spec(t, blocks, ("gemm", t, R, C))
    rows = permutation(R, R + t) if gather else None
    if rows is not None:
        want = want[rows.long()]
    return upload(blocks, 2 if t == NL else 8), (rows.cuda() if gather else None), want


def reference(want32, dt):
    """The spec's weight in the operand dtype, with the property that lets the comparison exclude nothing: no 16-bit
    subnormal, nothing non-finite (|d| in [2^-10, 2^-1): magnitudes 2^-10 .. 2032, or 0)."""
    want = want32.to(dt).cuda()
    assert bool(torch.isfinite(want).all()) and not bool(subnormal(want).any())
    nz = want32[want32 != 0].abs()
    assert float(nz.min()) >= 2.0 ** -10 and float(nz.max()) <= 2032.0
    return want


def same_values(y, want):
    """Every element equal, bit for bit wherever the weight is not zero.  An IQ4_XS weight with ls == 32 is d * 0 = -0 for a
    negative d and the decoder writes that sign; a sum of products that starts from +0 cannot return -0, so a zero weight is
    compared by value.  Nothing is left out: every element is compared."""
    y, want = y.contiguous(), want.contiguous()
    nz = want != 0
    return bool((y == want).all()) and torch.equal(bits(y)[nz], bits(want)[nz])


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("t", [XS, NL], ids=["IQ4_XS", "IQ4_NL"])
def test_identity_activations_reproduce_the_spec(ops, t, dt):  # noqa: F811
    """x = I: the tile kernel's result for [130, 512] and the GEMV's sixteen rows at a time for [20, 512] are the decoded weight
    transposed, every element of it."""
    C = 512
    eye = torch.eye(C, dtype=dt, device="cuda")
    src, rows, want32 = gemm_weight(t, 130, C, gather=(t == XS))
    want = reference(want32, dt)
    y = ops.linear_packed(t, src, eye, rows)
    assert y.shape == (C, 130) and y.dtype == dt
    assert same_values(y.T, want), f"{int((y.T != want).sum())} of {want.numel()} values differ"
    src, rows, want32 = gemm_weight(t, 20, C, gather=(t == NL))
    want = reference(want32, dt)
    y = torch.cat([ops.gemv_packed(t, src, eye[g:g + 16], rows) for g in range(0, C, 16)])
    assert same_values(y.T, want), f"{int((y.T != want).sum())} of {want.numel()} values differ"


@pytest.mark.parametrize("t", [XS, NL], ids=["IQ4_XS", "IQ4_NL"])
def test_one_hot_rows_reproduce_the_spec_at_one_token(ops, t):  # noqa: F811
    src, rows, want32 = gemm_weight(t, 20, 512, gather=(t == NL))
    want = reference(want32, F16)
    eye = torch.eye(512, dtype=F16, device="cuda")
    for c in (0, 15, 16, 31, 32, 255, 256, 511):  # first and last column of a lane, of a block of 32, of a superblock, of the row
        y = ops.gemv_packed(t, src, eye[c:c + 1], rows)
        assert y.shape == (1, 20) and same_values(y[0], want[:, c]), c
        y = ops.linear_packed(t, src, eye[c:c + 1], rows)
        assert same_values(y[0], want[:, c]), c


# (kernel, T, R): the GEMV at one token, a few and its maximum on a 16-row group and a partial one; the tile kernel on partial
# tiles both ways
RANDOM = [("gemv", 1, 20), ("gemv", 3, 20), ("gemv", 16, 20), ("tile", 17, 130)]
CASES = [(k, T, R, t, (F16, BF16)[(i + j) % 2]) for i, (k, T, R) in enumerate(RANDOM) for j, t in enumerate((XS, NL))]
CASE_IDS = [f"{c[0]}-T{c[1]}-R{c[2]}-{S.NAME[c[3]]}-{str(c[4])[6:]}" for c in CASES]
_case = {}


def case(kernel, T, R, t, dt):
    """Inputs, the kernel's result (in guarded memory), fp64 and the bound of one case, computed once.
    bound = u |y64| + C 2^-23 (|x| |Wd|^T) + 2^-25 per element, test_gpu_qgemm.py's: the final rounding (u = 2^-11 fp16, 2^-8
    bf16) plus the worst-case fp32 accumulation of C terms in any order.  Derived, not measured."""
    key = (kernel, T, R, t, dt)
    if key not in _case:
        C = 512
        src, rows, want32 = gemm_weight(t, R, C, gather=(R == 20))
        Wd = reference(want32, dt)
        x = torch.randn(T, C, generator=torch.Generator().manual_seed(T + R)).to(dt).cuda()
        buf, y = guarded_y(T, R, dt)
        (raw_gemv if kernel == "gemv" else raw_linear)(t, src, rows, R, C, x, T, y)
        y64 = x.double() @ Wd.double().T
        u = 2.0 ** -11 if dt == F16 else 2.0 ** -8
        bound = u * y64.abs() + C * 2.0 ** -23 * (x.double().abs() @ Wd.double().abs().T) + 2.0 ** -25
        _case[key] = dict(src=src, rows=rows, x=x, buf=buf, y=y, y64=y64, bound=bound)
    return _case[key]


@pytest.mark.parametrize("kernel,T,R,t,dt", CASES, ids=CASE_IDS)
def test_random_activations_against_fp64(ops, kernel, T, R, t, dt):  # noqa: F811
    c = case(kernel, T, R, t, dt)
    err = (c["y"].double() - c["y64"]).abs()
    worst = float((err / c["bound"]).max())
    print(f"{kernel} T={T} R={R} {S.NAME[t]} {dt}: max err / bound = {worst:.3f}")
    assert guards_intact(c["buf"]), "written outside [y, y + T * R * 2)"
    assert bool(torch.isfinite(c["y"]).all()) and float(c["y"].float().abs().max()) > 0
    assert bool((err <= c["bound"]).all()), f"max err / bound = {worst}"


@pytest.mark.parametrize("kernel,T,R,t,dt", CASES, ids=CASE_IDS)
def test_the_same_call_gives_the_same_bits_and_the_two_kernels_agree(ops, kernel, T, R, t, dt):  # noqa: F811
    """Both kernels lie within `bound` of the same fp64 value, so within 2 bound of each other."""
    c = case(kernel, T, R, t, dt)
    mine, other = (ops.gemv_packed, ops.linear_packed) if kernel == "gemv" else (ops.linear_packed, None)
    again = mine(t, c["src"], c["x"], c["rows"])
    assert torch.equal(bits(again), bits(c["y"]))
    if other is not None:
        tile = other(t, c["src"], c["x"], c["rows"])
        diff = (c["y"].double() - tile.double()).abs()
        print(f"gemv T={T} R={R} {S.NAME[t]} {dt}: max |gemv - linear_packed| / bound = {float((diff / c['bound']).max()):.3f}")
        assert bool((diff <= 2 * c["bound"]).all())


# ------------------------------------------------------------------------------------------------ 4: the grouped kernels
E, ER, EC = 3, 20, 256
PAIRS = {"T1-K2": (1, 2, [1, 0]), "T9-K2": (9, 2, [0, 1] * 5 + [1, 0] * 4), "masked": (3, 2, [0, 1, E, 0, 1, 0])}  # expert 2: unnamed


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("t", [XS, NL], ids=["IQ4_XS", "IQ4_NL"])
def test_grouped_kernels_equal_the_single_matrix_kernels_on_the_experts_slice(ops, t, dt):  # noqa: F811
    """Row p of gemv_packed_experts is gemv_packed, and of linear_packed_experts linear_packed, of expert pair_expert[p]'s
    slice and x[p // pairs_per_row]: torch.equal on the bits.  A masked pair's row stays as it was."""
    from gptq_gguf_toolkit_amd import _cabi
    from gptq_gguf_toolkit_amd.ops import _DT, _ptr, _stream
    src = upload(S.gemm_fixture(t, E * ER, EC), 2 if t == NL else 8)
    slices = src.view(E, -1)
    L = _cabi.lib()
    for name, (x_rows, ppr, ids) in PAIRS.items():
        x = torch.randn(x_rows, EC, generator=torch.Generator().manual_seed(x_rows)).to(dt).cuda()
        pe = torch.tensor(ids, dtype=torch.int32, device="cuda")
        route = ops.moe_route(pe, E)
        buf_v, yv = guarded_y(len(ids), ER, dt)
        buf_m, ym = guarded_y(len(ids), ER, dt)
        assert L.gq_gemv_packed_experts(t, _ptr(src), E, ER, EC, _ptr(x), x_rows, _ptr(pe), len(ids), ppr, _DT[dt], _ptr(yv),
                                        _stream(x)) == 0, L.gq_last_error()
        assert L.gq_linear_packed_experts(t, _ptr(src), E, ER, EC, _ptr(x), x_rows, ppr, _ptr(route[0]), _ptr(route[1]), len(ids),
                                          _DT[dt], _ptr(ym), _stream(x)) == 0, L.gq_last_error()
        for p, e in enumerate(ids):
            if e >= E:
                assert bool((bits(yv[p]) == FILL).all()) and bool((bits(ym[p]) == FILL).all()), (name, p)
                continue
            xr = x[p // ppr:p // ppr + 1]
            assert torch.equal(bits(yv[p]), bits(ops.gemv_packed(t, slices[e], xr)[0])), (name, p, e)
            assert torch.equal(bits(ym[p]), bits(ops.linear_packed(t, slices[e], xr)[0])), (name, p, e)
        assert guards_intact(buf_v) and guards_intact(buf_m), name
        named = [p for p, e in enumerate(ids) if e < E]
        assert bool(torch.isfinite(yv[named]).all()) and float(yv[named].float().abs().max()) > 0
        if name != "masked":  # the bindings: the same calls
            assert torch.equal(bits(ops.gemv_packed_experts(t, src, E, ER, x, pe, ppr)), bits(yv))
            assert torch.equal(bits(ops.linear_packed_experts(t, src, E, ER, x, route, ppr)), bits(ym))


# ------------------------------------------------------------------------------------------------ 5: a model
LINEARS = r"((q|k|v|o|gate|up|down)_proj)$"
NL_TENSOR = "blk.1.attn_k.weight"  # the one IQ4_NL tensor: a gathered one


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The tiny Llama (hidden 256, 2 layers, 4 / 2 heads, vocab 512) as a .gguf written by tests/gguf_spec_writer.py: its
    fourteen Linears as IQ4_XS blocks (one as IQ4_NL) of weights around 0.03 rms, everything else from the seeded model."""
    import gguf_spec_writer as W
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import map_tensor_name
    tmp = tmp_path_factory.mktemp("iq4model")
    model = tiny_llama(dtype=F16)
    tensors, stored = [], {}
    for i, (name, w) in enumerate(model.state_dict().items()):
        g = map_tensor_name(name)
        if re.search(LINEARS, name.rsplit(".", 1)[0]):
            t = NL if g == NL_TENSOR else XS
            blocks = S.model_blocks(t, w.shape[0], w.shape[1], seed=700 + i)
            stored[name] = (g, t, blocks)
            tensors.append((g, tuple(w.shape), S.NAME[t], blocks.tobytes()))
        elif w.dim() == 1:
            tensors.append((g, tuple(w.shape), "F32", w.float().numpy().tobytes()))
        else:
            tensors.append((g, tuple(w.shape), "F16", w.numpy().tobytes()))
    assert len(stored) == 14 and sum(t == NL for _, t, _ in stored.values()) == 1
    kvs = [("general.architecture", "str", "llama"), ("llama.attention.head_count", "u32", 4),
           ("llama.attention.head_count_kv", "u32", 2)]
    path = tmp / "iq4.gguf"
    path.write_bytes(W.serialise(kvs, tensors))
    return dict(tmp=tmp, path=str(path), stored=stored, ids=tiny_calib()[0].cuda(), tiny_llama=tiny_llama)


def test_the_file_loads_dense_and_packed(world):
    from gptq_gguf_toolkit_amd import gguf_loader
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    tiny_llama = world["tiny_llama"]
    dense = gguf_loader.load_into_model(tiny_llama(seed=123, dtype=F16).cuda(), world["path"])
    packed = gguf_loader.load_into_model(tiny_llama(seed=321, dtype=F16).cuda(), world["path"], packed=True)
    for name, (g, t, blocks) in world["stored"].items():
        want = torch.from_numpy(S.decode(t, blocks)).to(F16)
        assert bool(torch.isfinite(want).all()) and not bool(subnormal(want).any()) and 0.01 < float(want.float().std()) < 0.1
        if g.endswith(".attn_q.weight"):
            want = gguf_loader.unpermute(want, 4, 4)
        elif g.endswith(".attn_k.weight"):
            want = gguf_loader.unpermute(want, 4, 2)
        got = dense.state_dict()[name]
        assert torch.equal(bits(got.cpu()), bits(want)), f"{name}: {int((bits(got.cpu()) != bits(want)).sum())} values differ"
        m = packed.get_submodule(name.rsplit(".", 1)[0])
        assert type(m) is PackedLinear and m.q_type == t, name
        assert (m.row_src is not None) == name.endswith(("q_proj.weight", "k_proj.weight")), name
        assert torch.equal(bits(m.dense_weight()), bits(got)), name
    for k, w in packed.state_dict().items():  # embeddings, norms and lm_head load as without the flag
        assert torch.equal(bits(w), bits(dense.state_dict()[k])), k
    ids = world["ids"]
    with torch.no_grad():
        got, want = packed(ids).logits.float(), dense(ids).logits.float()
        ref = copy.deepcopy(dense).float()(ids).logits
    # The yardstick of the packed-model tests (test_gpu_packed_vocab.py, test_gpu_generate.py): floor = the dense 16-bit
    # forward against the same weights in fp32, measured on the dense model; the packed path shares its roundings and differs
    # in fp32 summation order only, and two independently rounded 16-bit runs may land on opposite sides of the reference.
    floor, err = float((want - ref).abs().max()), float((got - ref).abs().max())
    print(f"64 x 512 logits against fp32: dense {floor!r}, packed {err!r}; max |logit| {float(ref.abs().max())!r}")
    assert bool(torch.isfinite(got).all()) and float(ref.abs().max()) > 0
    assert err <= 2 * floor


def test_level_store_switches_between_q4_k_and_iq4_xs(world, ops):  # noqa: F811
    """A --gguf-layers database with a Q4_K level (RTN of the model's weights) and an IQ4_XS level per Linear: both residencies
    switch between them and hold what level_db.load_level decodes."""
    from gptq_gguf_toolkit_amd import level_db
    from gptq_gguf_toolkit_amd.gguf_writer import GGUFWriter, kv_records
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import map_tensor_name
    from gptq_gguf_toolkit_amd.packed_linear import PackedLinear
    base = world["tiny_llama"](dtype=F16).cuda()
    names = [n for n, m in base.named_modules() if isinstance(m, torch.nn.Linear) and re.search(LINEARS, n)]
    db = world["tmp"] / "db"
    w = GGUFWriter(str(world["tmp"] / "unused.gguf"), "llama")
    w.add_uint32("llama.attention.head_count", 4)
    w.add_uint32("llama.attention.head_count_kv", 2)
    with level_db.LevelDbWriter(str(db)) as wr:
        for i, n in enumerate(names):
            W = base.get_submodule(n).weight.data
            g = map_tensor_name(n + ".weight")
            wr.add_level(g, tuple(W.shape), 12, ops.pack(12, *ops.rtn_quantize(W.float(), 12)).cpu().numpy())
            wr.add_level(g, tuple(W.shape), XS, S.model_blocks(XS, W.shape[0], W.shape[1], seed=900 + i))
        wr.set_metadata(kv_records(w.kv))
    levels = level_db.scan_available_bitwidths(str(db), names)
    assert all([k for k, _ in v] == [4.25, 4.5] for v in levels.values())
    dense_model, packed_model = copy.deepcopy(base), copy.deepcopy(base)
    dense, packed = LevelStore(dense_model, str(db), "cuda"), LevelStore(packed_model, str(db), "cuda", resident="packed")
    states = [{n: (4.25, 4.5)[(i + flip) % 2] for i, n in enumerate(names)} for flip in (0, 1)]
    for state in states + states[:1]:
        assert dense.switch(state) == 14 and packed.switch(state) == 14
        for n in names:
            path = level_db.find_level_file(level_db.layer_dir(str(db), n), state[n])
            want = level_db.load_level(path, "cuda", str(db))
            assert want.dtype == F16 and bool(torch.isfinite(want).all())
            assert torch.equal(bits(dense_model.get_submodule(n).weight.data), bits(want)), (n, state[n])
            m = packed_model.get_submodule(n)
            assert type(m) is PackedLinear and m.q_type == (XS if state[n] == 4.25 else 12)
            assert torch.equal(bits(m.dense_weight()), bits(want)), (n, state[n])
    assert packed.jobs_issued == 0 and dense.jobs_issued > 0
    ids = world["ids"]
    with torch.no_grad():
        a, b = packed_model(ids).logits, dense_model(ids).logits
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
