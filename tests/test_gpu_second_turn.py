"""-m gpu: every capped-grid streaming kernel through a second (and third) turn of its grid-stride loop.  The other files pin
these kernels bit for bit at shapes below their grid caps, where no workgroup ever re-enters its loop: the block bookkeeping
after `b0 += gridDim.x * per_turn`, the reuse of the LDS image behind the trailing barrier and a ragged last turn that is not
the first one run here.  Every equality is on bits.  Each large case has three anchors: the whole call equals the same kernel on
row ranges that stay at or below the cap (one-turn behaviour is pinned to the specs elsewhere); the last ten rows -- they hold
every block of the turns past the cap -- equal the CPU spec or host form; 64 guard bytes on either side of the output survive a
call whose last turn is partial.  The shapes, with their arithmetic, live in tests/test_second_turn_shapes_cpu.py, which also reads the
cap literals from csrc/ so that a changed cap fails there instead of turning this file into a one-turn test:

  kernel (file)                                                   units per turn      cap     shape here
  q8_0_encode_kernel (q8/gq_q8_0.hip)                             128 blocks of 32    16384   [16260, 4128]: 16388 turns, 4 blocks last
  dequantize_b32_kernel Q8_0 / IQ4_NL (decode/gq_decode.hip)      128 blocks of 32    16384   the same
  dequantize_blocks_kernel, unpack_kernel (decode/gq_decode.hip)  16 blocks of 256    16384   [29134, 2304]: 16388 turns, 14 last
  pack_kernel (gq_codec.hip)                                      32 blocks of 256    4096    the same: 8194 turns, 30 last
  dequantize_kernel (gq_codec.hip)                                256 x 16 values     8192    the same: 2 passes and a partial third
  iq4_pack_kernel (iq4/gq_iq4_gptq.hip)                           256 blocks of 32    4096    XS [14569, 2304], NL [8132, 4128]: 4098 turns
  iq4_encode_kernel IQ4_XS (iq4/gq_iq4_encode.hip)                256 blocks of 32    4096    XS [14569, 2304]
  fwd_silu_mul_kernel (gq_forward.hip)                            256 x 8 values      16384   2^25 + 8 x 777 values: 9 lanes last
  fwd_moe_combine_kernel (calib/gq_moe_combine.hip)               one token           2048    T = 4101 and 2053; H / 8 = 65, 129, 513
  stage_rows / stage_bytes / stage_many_kernel (gq_hessian.hip)   16 KiB / 256 B      4096 / 4096 / 2048 (1 for the host copy)

Measured wall time of this file on an MI355X: 7.2 s for its 58 tests, the slowest 0.4 s (the host-side combine_spec loop over 4101
tokens); the largest tensors are 268 MB."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests"))

import iq4_encode_spec  # noqa: E402
import iq4_spec  # noqa: E402
import test_moe_quantize_cpu as moe_host  # noqa: E402
import test_second_turn_shapes_cpu as shapes  # noqa: E402
from moe_combine_spec import combine_hf, combine_spec, route, transposed_pairs  # noqa: E402
from test_gpu_decode import D_AT, TYPES, assert_fields, formula_f32, random_blocks, spec_unpack  # noqa: E402
from test_gpu_q8 import q8_bytes, torch_decode  # noqa: E402

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = (F32, F16, BF16)
DT_ID = {F32: "f32", F16: "f16", BF16: "bf16"}
AS_INT = {4: torch.int32, 2: torch.int16, 1: torch.uint8}
Q8, NL, XS = 8, iq4_spec.NL, iq4_spec.XS
PROBE = shapes.PROBE_ROWS
GUARD, SENTINEL = 64, 0xA5
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from gptq_gguf_toolkit_amd import ops as _ops
    return _ops


def bits(t):
    return t.contiguous().view(AS_INT[t.element_size()])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def shape_of(name):
    """(R, C, rows of the first part) of a table entry, with the facts the tests below rely on re-asserted."""
    s = shapes.SHAPES[name]
    units, n_turns, rest = shapes.turns(name)
    assert n_turns > s["cap"] and 0 < rest < s["per_turn"], shapes.REDERIVE
    return s["R"], s["C"], (s["parts"][0] if s["parts"] else None)


class Guarded:
    """`nbytes` of device memory with 64 sentinel bytes on either side; .mid is the 16-byte aligned window a kernel writes."""

    def __init__(self, nbytes):
        self.buf = torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.mid = self.buf[GUARD:GUARD + nbytes]

    @property
    def ptr(self):
        return vp(self.mid.data_ptr())

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[-GUARD:] == SENTINEL).all())

    def holds(self, t):
        """The window equals tensor t byte for byte and the guards are as they were."""
        return self.intact() and torch.equal(self.mid, t.contiguous().view(-1).view(torch.uint8))


def call(name, *args):
    from gptq_gguf_toolkit_amd import _cabi
    _cabi.check(getattr(_cabi.lib(), name)(*args), name)


def device_blocks(n, ts, d_at, seed, clear=0xFB, subnormal_every=0):
    """The device twin of test_gpu_decode.random_blocks / test_gpu_q8.q8_bytes / iq4_spec.blocks_with_d: n blocks of ts uniformly
    random bytes whose fp16 fields at the byte offsets d_at are forced finite by the helpers' own rule (an exponent of 31 loses
    the bit `~clear` of the high byte: 30 for the K-quants and IQ4, 15 for Q8_0); every `subnormal_every`-th an fp16 subnormal."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    b = torch.randint(0, 256, (n, ts), dtype=torch.uint8, device="cuda", generator=g)
    for off in d_at:
        hi = b[:, off + 1]
        b[:, off + 1] = torch.where((hi & 0x7C) == 0x7C, hi & clear, hi)
        if subnormal_every:
            b[::subnormal_every, off + 1] &= 0x83
        assert bool(torch.isfinite(b[:, off:off + 2].contiguous().view(F16)).all())
    return b


def permutation(R, seed):
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(seed)).to(torch.int32).cuda()
    assert not torch.equal(perm[-PROBE:].cpu(), torch.arange(R - PROBE, R, dtype=torch.int32))
    return perm


def check_dequantize_blocks(ops, t, raw, R, C, half, perm, probe_f32, dt):
    """gq_dequantize_blocks of the whole [R, C] in `dt`: == the two parts; the probe rows == the spec's fp32 values, cast once;
    row_src == a gather of the plain result; the call through the C ABI leaves its guards alone.  -> the plain result."""
    whole = ops.dequantize_blocks(t, raw, dt)
    assert whole.dtype == dt and tuple(whole.shape) == (R, C)
    assert torch.equal(bits(whole[:half]), bits(ops.dequantize_blocks(t, raw[:half], dt))), "first part"
    assert torch.equal(bits(whole[half:]), bits(ops.dequantize_blocks(t, raw[half:], dt))), "second part"
    assert torch.equal(bits(whole[-PROBE:]).cpu(), bits(torch.from_numpy(probe_f32).to(dt))), "probe rows"
    gathered = ops.dequantize_blocks(t, raw, dt, perm)
    assert torch.equal(bits(gathered), bits(whole[perm.long()])), "row_src"
    del gathered
    g = Guarded(R * C * whole.element_size())
    call("gq_dequantize_blocks", int(t), vp(raw.data_ptr()), R, C, vp(0), g.ptr, ops._DT[dt], stream())
    assert g.holds(whole), "guards"
    return whole


# ------------------------------------------------------------------------------------------------ 32-value blocks: Q8_0
@pytest.fixture(scope="module")
def b32_x():
    """fp32 [16260, 4128] on the device (some blocks all zero: d = 0), and a row permutation."""
    R, C, _ = shape_of("b32")
    g = torch.Generator(device="cuda").manual_seed(20)
    x = torch.randn(R, C, generator=g, device="cuda") * 3
    x.view(-1, 32)[::1001] = 0
    return x, permutation(R, 20)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.values())
def test_q8_0_encoder_past_the_grid_cap(ops, b32_x, dt):
    from gptq_gguf_toolkit_amd.gguf_writer import quantize_q8_0
    R, C, half = shape_of("b32")
    x32, perm = b32_x
    x = x32.to(dt)
    whole = ops.quantize_q8_0(x)
    assert whole.dtype == torch.uint8 and tuple(whole.shape) == (R, C // 32 * 34)
    assert torch.equal(whole[:half], ops.quantize_q8_0(x[:half])) and torch.equal(whole[half:], ops.quantize_q8_0(x[half:]))
    with np.errstate(over="ignore"):
        want = quantize_q8_0(x[-PROBE:].float().cpu().numpy())
    assert whole[-PROBE:].cpu().numpy().tobytes() == want.tobytes()
    gathered = ops.quantize_q8_0(x, perm)
    assert torch.equal(gathered, whole[perm.long()]) and not torch.equal(gathered[-PROBE:], whole[-PROBE:])
    with np.errstate(over="ignore"):
        want = quantize_q8_0(x[perm[-PROBE:].long()].float().cpu().numpy())
    assert gathered[-PROBE:].cpu().numpy().tobytes() == want.tobytes()
    del gathered
    g = Guarded(whole.numel())
    call("gq_quantize_q8_0", vp(x.data_ptr()), ops._DT[dt], R, C, vp(0), g.ptr, stream())
    assert g.holds(whole)


@pytest.fixture(scope="module")
def b32_q8_raw():
    R, C, _ = shape_of("b32")
    raw = device_blocks(R * (C // 32), 34, (0,), seed=21, clear=0xBF, subnormal_every=7).view(R, -1)
    host = q8_bytes(PROBE, C, seed=22)  # the probe rows are the host helper's: -0, +0 and subnormal d included
    raw[-PROBE:] = torch.from_numpy(host).cuda()
    return raw, host, permutation(R, 21)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.values())
def test_q8_0_decoder_past_the_grid_cap(ops, b32_q8_raw, dt):
    from ggml_spec import q8_0_decode
    R, C, half = shape_of("b32")
    raw, host, perm = b32_q8_raw
    probe = q8_0_decode(host.tobytes(), PROBE * C).reshape(PROBE, C)
    whole = check_dequantize_blocks(ops, Q8, raw, R, C, half, perm, probe, dt)
    assert torch.equal(bits(whole), bits(torch_decode(raw, R, C, None, dt)))
    del whole
    assert torch.equal(bits(ops.dequantize_blocks(Q8, raw, dt, perm)), bits(torch_decode(raw, R, C, perm, dt)))


# ------------------------------------------------------------------------------------------------ 32-value blocks: IQ4_NL
@pytest.fixture(scope="module")
def b32_nl_raw():
    R, C, _ = shape_of("b32")
    raw = device_blocks(R * (C // 32), 18, (0,), seed=23, subnormal_every=7).view(R, -1)
    host = iq4_spec.blocks_with_d(NL, PROBE, C, seed=24)
    raw[-PROBE:] = torch.from_numpy(host).cuda()
    return raw, iq4_spec.decode(NL, host), permutation(R, 23)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.values())
def test_iq4_nl_decoder_past_the_grid_cap(ops, b32_nl_raw, dt):
    R, C, half = shape_of("b32")
    raw, probe, perm = b32_nl_raw
    check_dequantize_blocks(ops, NL, raw, R, C, half, perm, probe, dt)


# ------------------------------------------------------------------------------------------------ 256-value blocks
B256 = dict(TYPES, IQ4_XS=XS)
B256_TS = {10: 84, 11: 110, 12: 144, 13: 176, 14: 210, XS: 136}
B256_D_AT = dict(D_AT)
B256_D_AT[XS] = (0,)


def b256_case(t):
    """(type, blocks uint8 [29134, 9 * type_size] on the device, the host copy of the probe rows, a row permutation)."""
    R, C, _ = shape_of("b256")
    raw = device_blocks(R * (C // 256), B256_TS[t], B256_D_AT[t], seed=30 + t).view(R, -1)
    host = iq4_spec.blocks_with_d(XS, PROBE, C, seed=31) if t == XS else random_blocks(t, PROBE, C // 256, seed=31 + t)
    raw[-PROBE:] = torch.from_numpy(host).cuda()
    return t, raw, host, permutation(R, 30 + t)


@pytest.fixture(params=list(B256))
def b256(request):
    return b256_case(B256[request.param])


@pytest.fixture(params=list(TYPES))  # IQ4_XS has no gq_unpack / gq_pack / gq_dequantize form: its own packer is tested below
def k256(request):
    return b256_case(TYPES[request.param])


def test_block_decoder_past_the_grid_cap(ops, b256):
    t, raw, host, perm = b256
    R, C, half = shape_of("b256")
    probe = iq4_spec.decode(XS, host) if t == XS else formula_f32(t, spec_unpack(t, host))
    assert np.isfinite(probe).all()
    for dt in DTYPES:
        check_dequantize_blocks(ops, t, raw, R, C, half, perm, probe, dt)


def unpack_guarded(ops, t, raw, R, C):
    from gptq_gguf_toolkit_amd._cabi import type_info
    G = type_info(t)["group"]
    outs = [Guarded(n) for n in (R * C, R * (C // 256) * 2, R * (C // G), R * (C // 256) * 2, R * (C // G))]
    call("gq_unpack", int(t), vp(raw.data_ptr()), R, C, *[o.ptr for o in outs], stream())
    return outs


def test_unpack_pack_and_dequantize_past_their_grid_caps(ops, k256):
    t, raw, host, _ = k256
    R, C, half = shape_of("b256")
    fields = ops.unpack(t, raw)
    for name, lo, hi in (("first part", 0, half), ("second part", half, R)):
        part = ops.unpack(t, raw[lo:hi])
        assert all(same(a[lo:hi], b) for a, b in zip(fields, part)), name
        del part
    assert_fields(tuple(f[-PROBE:] for f in fields), *spec_unpack(t, host))
    outs = unpack_guarded(ops, t, raw, R, C)
    for k, (o, f) in enumerate(zip(outs, fields)):
        assert o.holds(f), k  # (Q3_K / Q6_K: dmin and m are written too, as zeros)
    del outs
    # the packer: 8194 turns of 32 blocks over 4096 workgroups; the random bytes are the reference
    _, n_turns, rest = shapes.turns("pack")
    assert n_turns > 2 * shapes.SHAPES["pack"]["cap"] and rest == 30
    assert torch.equal(ops.pack(t, *fields), raw)
    g = Guarded(raw.numel())
    call("gq_pack", int(t), *[vp(f.data_ptr()) for f in fields], R, C, g.ptr, stream())
    assert g.holds(raw)
    del g
    # the field dequantizer: two full passes of the 8192 x 256 x 16 grid and a partial third
    assert R * C == 67124736
    for dt in DTYPES:
        want = ops.dequantize_blocks(t, raw, dt)
        assert torch.equal(bits(ops.dequantize(t, *fields, out_dtype=dt)), bits(want)), dt
        g = Guarded(R * C * want.element_size())
        call("gq_dequantize", int(t), *[vp(f.data_ptr()) for f in fields], R, C, g.ptr, ops._DT[dt], stream())
        assert g.holds(want), dt
        del g, want


# ------------------------------------------------------------------------------------------------ the IQ4 packer
def iq4_fields(t, R, C, seed):
    """Random outputs of the column walk: codes 0 .. 15, any finite fp16 d, ls 0 .. 63 (IQ4_XS)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randint(0, 16, (R, C), dtype=torch.uint8, device="cuda", generator=g)
    nd = C // 256 if t == XS else C // 32
    d = device_blocks(R * nd, 2, (0,), seed + 1, subnormal_every=7).view(F16).view(R, nd)
    ls = torch.randint(0, 64, (R, C // 32), dtype=torch.uint8, device="cuda", generator=g) if t == XS else None
    return q, d, ls


def iq4_formula(t, q, d, ls):
    """kvalues[code] * d * (ls - 32) in numpy fp32, the way tests/iq4_spec.py states it: dl = d * (ls - 32), then dl * kv."""
    kv = np.array(iq4_spec.KV, np.float32)[q.cpu().numpy()]
    d32 = d.cpu().numpy().astype(np.float32)
    if t == XS:
        dl = np.repeat(d32, 8, axis=1) * (ls.cpu().numpy().astype(np.float32) - np.float32(32))
    else:
        dl = d32
    return np.repeat(dl, 32, axis=1) * kv


@pytest.mark.parametrize("name", ["iq4_xs", "iq4_nl"])
def test_iq4_packer_past_the_grid_cap(ops, name):
    t = XS if name == "iq4_xs" else NL
    R, C, half = shape_of(name)
    bs, ts = iq4_spec.GEOMETRY[t]
    q, d, ls = iq4_fields(t, R, C, seed=40 + t)
    cut = lambda lo, hi: (q[lo:hi], d[lo:hi], None if ls is None else ls[lo:hi])  # noqa: E731
    whole = ops.pack_iq4(t, q, d, ls)
    assert whole.dtype == torch.uint8 and tuple(whole.shape) == (R, C // bs * ts)
    assert torch.equal(whole[:half], ops.pack_iq4(t, *cut(0, half))) and torch.equal(whole[half:], ops.pack_iq4(t, *cut(half, R)))
    got = iq4_spec.decode(t, whole[-PROBE:].cpu().numpy())
    assert np.array_equal(got.view(np.uint32), iq4_formula(t, *cut(R - PROBE, R)).view(np.uint32))
    perm = permutation(R, 40 + t)
    gathered = ops.pack_iq4(t, q, d, ls, perm)
    assert torch.equal(gathered, whole[perm.long()]) and not torch.equal(gathered[-PROBE:], whole[-PROBE:])
    for rows in (None, perm):
        g = Guarded(whole.numel())
        assert ops.pack_iq4(t, q, d, ls, rows, out=g.mid).data_ptr() == g.mid.data_ptr()
        assert g.holds(whole if rows is None else gathered)


# ------------------------------------------------------------------------------------------------ the IQ4_XS encoder
@pytest.mark.parametrize("dt", [F32, F16], ids=["f32", "f16"])
def test_iq4_xs_encoder_past_the_grid_cap(ops, dt):
    from gptq_gguf_toolkit_amd.gguf_writer import quantize_iq4
    R, C, half = shape_of("iq4_xs")
    g = torch.Generator(device="cuda").manual_seed(50)
    x = (torch.randn(R, C, generator=g, device="cuda") * 0.03).to(dt)
    imp = torch.from_numpy(iq4_encode_spec.random_importance(C, seed=50)).cuda()
    whole = ops.quantize_iq4(x, XS, imp)
    assert whole.dtype == torch.uint8 and tuple(whole.shape) == (R, C // 256 * 136)
    assert torch.equal(whole[:half], ops.quantize_iq4(x[:half], XS, imp)), "first part"
    assert torch.equal(whole[half:], ops.quantize_iq4(x[half:], XS, imp)), "second part"
    want = quantize_iq4(x[-PROBE:].float().cpu().numpy(), XS, imp.cpu().numpy())
    assert whole[-PROBE:].cpu().numpy().tobytes() == want.tobytes()
    guard = Guarded(whole.numel())
    ops.quantize_iq4(x, XS, imp, out=guard.mid)
    assert guard.holds(whole)


# ------------------------------------------------------------------------------------------------ silu(gate) * up
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_silu_mul_past_the_grid_cap(ops, dt):
    _, n, _ = shape_of("silu")
    assert n == 33554432 + 8 * 777
    g = torch.Generator(device="cuda").manual_seed(60)
    gate = (torch.randn(n, generator=g, device="cuda") * 3).to(dt)
    up = torch.randn(n, generator=g, device="cuda").to(dt)
    want = torch.nn.functional.silu(gate) * up
    assert torch.equal(bits(ops.fwd_silu_mul(gate, up)), bits(want))
    guard = Guarded(n * 2)
    call("gq_fwd_silu_mul", vp(gate.data_ptr()), vp(up.data_ptr()), guard.ptr, n, ops._DT[dt], stream())
    assert guard.holds(want)


# ------------------------------------------------------------------------------------------------ the MoE combine
def run_combine(ops, y, idx, w, E):
    """test_gpu_moe_quantize.run_kernel for any E: the route on the device (== the loop restatement), then the combine through
    the binding and once more through the C ABI into a guarded buffer."""
    T, K = idx.shape
    H = y.shape[1]
    pairs = idx.t().contiguous().view(-1).to(torch.int32).cuda()
    rt = ops.moe_route(pairs, E)
    start, order = route(transposed_pairs(idx), E)
    assert rt[0].tolist() == start and rt[1].tolist() == order
    yd, wd = y.cuda(), w.cuda()
    out = ops.fwd_moe_combine(yd, pairs, rt, wd, E)
    assert out.dtype == y.dtype and tuple(out.shape) == (T, H)
    g = Guarded(T * H * 2)
    call("gq_fwd_moe_combine", vp(yd.data_ptr()), vp(pairs.data_ptr()), vp(rt[0].data_ptr()), vp(rt[1].data_ptr()),
         vp(wd.data_ptr()), ops._DT[w.dtype], T, K, E, H, ops._DT[y.dtype], g.ptr, stream())
    assert g.holds(out)
    return out


COMBINE_DTYPES = [(dt, w_kind) for dt in (F16, BF16) for w_kind in ("w-fp32", "w-act")]


@pytest.mark.parametrize("T,K,E,H", shapes.COMBINE_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("dt,w_kind", COMBINE_DTYPES, ids=[f"{DT_ID[dt]}-{k}" for dt, k in COMBINE_DTYPES])
def test_combine_past_the_grid_cap_and_in_every_block_size(ops, dt, w_kind, T, K, E, H):
    w_dt = F32 if w_kind == "w-fp32" else dt
    y, idx, w = moe_host.combine_case(T, K, E, H, dt, w_dt, seed=T + K + H)
    got = run_combine(ops, y, idx, w, E)
    assert torch.equal(bits(got.cpu()), bits(combine_spec(y, idx, w, E)))
    if K <= 2:  # no token names an expert twice: transformers' result, bit for bit
        assert all(len(set(row)) == K for row in idx.tolist())
        assert torch.equal(bits(got), bits(combine_hf(y.cuda(), idx.cuda(), w.cuda(), E)))


@pytest.mark.parametrize("dt,w_kind", COMBINE_DTYPES, ids=[f"{DT_ID[dt]}-{k}" for dt, k in COMBINE_DTYPES])
def test_combine_edges_on_a_workgroups_later_tokens(ops, dt, w_kind):
    """An unused expert, masked pairs, a token with every pair masked and a first product of -0, the last three on tokens that
    a workgroup reaches on its second turn (combine_case itself puts a -0 on token 0, a first turn)."""
    e = shapes.COMBINE_EDGE
    T, K, E, H = e["T"], e["K"], e["E"], e["H"]
    w_dt = F32 if w_kind == "w-fp32" else dt
    y, idx, w = moe_host.combine_case(T, K, E, H, dt, w_dt, seed=1, unused=e["unused"], masked=e["masked"],
                                      all_masked=e["all_masked"], neg_zero=True)
    t0 = e["neg_zero_token"]
    idx[t0, 1:] = E  # this token keeps its first pair only, and that product is -0 in element 0 (w > 0)
    order = route(transposed_pairs(idx), E)[1]  # (one pair fewer than combine_case routed: token 0's row has moved as well)
    for t in (0, t0):
        assert int(idx[t, 0]) < E and float(w[t, 0]) > 0
        y[order.index(t), 0] = -0.0  # pair (t, k = 0) is p = t
        assert int(bits(y)[order.index(t), 0]) == -0x8000
    got = run_combine(ops, y, idx, w, E)
    assert torch.equal(bits(got.cpu()), bits(combine_spec(y, idx, w, E)))
    assert torch.equal(bits(got), bits(combine_hf(y.cuda(), idx.cuda(), w.cuda(), E)))
    out = bits(got.cpu())
    assert int(out[0, 0]) == 0 and int(out[t0, 0]) == 0  # +0, not the -0 of the product
    assert bool((out[e["all_masked"]] == 0).all())


# ------------------------------------------------------------------------------------------------ the staging copies
def pattern(n, dt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 251, (n,), device="cuda", generator=g).to(dt)


def test_stage_to_host_with_one_workgroup(ops):
    s = shapes.STAGE_HOST
    st = torch.cuda.current_stream()
    cases = ((s["byte_case"], torch.uint8), (s["row_case"][0] * s["row_case"][1], F16))
    with ops.options(stage_host_wgs=s["wgs"]):
        for k, (n, dt) in enumerate(cases):
            src = pattern(n, dt, 70 + k)
            es = src.element_size()
            host = torch.full((GUARD + n * es + GUARD,), SENTINEL, dtype=torch.uint8).pin_memory()
            dst = host[GUARD:GUARD + n * es].view(dt)
            ops.stage_to_host(dst, src, st)
            torch.cuda.synchronize()
            assert torch.equal(bits(dst), bits(src.cpu())), n
            assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[-GUARD:] == SENTINEL).all()), n
    assert ops.option_get("stage_host_wgs") == 0


@pytest.mark.parametrize("case", ["rows_case", "bytes_case"])
def test_h_stage_past_the_grid_cap(ops, case):
    s = shapes.STAGE
    T, C = s[case]
    fill = s["fill"]
    x = pattern(T * C, F16, 72).view(T, C)
    buf = torch.full((fill + T + 2, C), -7.0, dtype=F16, device="cuda")
    assert ((buf.data_ptr() + fill * C * 2) % 16 == 0) == (case == "rows_case")  # the 16-byte kernel / the byte kernel
    ops.h_stage(buf, fill, x)
    assert torch.equal(bits(buf[fill:fill + T]), bits(x))
    assert bool((buf[:fill] == -7.0).all()) and bool((buf[fill + T:] == -7.0).all())


def test_h_stage_many_past_the_grid_cap(ops):
    m = shapes.STAGE_MANY
    rows, C, fill = shapes.stage_many_rows(), m["C"], shapes.STAGE["fill"]
    total = sum(rows)
    assert m["total"][0] <= total <= m["total"][1] and total * C * 2 > (32 << 20) + (16 << 10) and len(rows) == m["blocks"]
    xs = [pattern(r * C, F16, 80 + k).view(r, C) for k, r in enumerate(rows)]
    buf = torch.full((fill + total + 2, C), -7.0, dtype=F16, device="cuda")
    ops.h_stage_many(buf, fill, xs)
    assert torch.equal(bits(buf[fill:fill + total]), bits(torch.cat(xs)))
    assert bool((buf[:fill] == -7.0).all()) and bool((buf[fill + total:] == -7.0).all())
