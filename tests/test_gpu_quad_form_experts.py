"""-m gpu: gq_quad_form_experts (K31) against the per-expert gq_quad_form loop, on the fp64 BITS.

The contract is equality, so there is no tolerance here: out[e] must be what ops.quad_form writes for A[e], H[e], B[e], and
that kernel's accuracy is pinned by tests/test_gpu_errest.py.  Shapes are the smallest at which the grouped launch can go
wrong: C = 128 (one column block: no doubling), 256 and 384 (doubling, and the tile order across column blocks and experts);
R = 1, 128 and 130 (one row, a full tile, a ragged second row tile); E = 1, 3, 5."""
import ctypes

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CS, RS, ES = (128, 256, 384), (1, 128, 130), (1, 3, 5)
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
E_MAX, R_MAX = max(ES), max(RS)


def _ops():
    from gptq_gguf_toolkit_amd import ops
    return ops


def _bits(t):
    return t.view(torch.int64)


_made = {}


def inputs(C):
    """(A fp32 [E_MAX, R_MAX, C], noise, H [E_MAX, C, C]) of a width, made once and left unchanged.  Expert e's Hessian comes
    from its own tokens (the package's SYRK); expert 1 saw none (H all zero), expert 2 has one dead channel at a diagonal
    position inside the last column block."""
    if C not in _made:
        g = torch.Generator(device="cuda").manual_seed(31 * C)
        H = torch.zeros(E_MAX, C, C, device="cuda")
        for e in range(E_MAX):
            if e == 1:
                continue
            T = C + 32 * e
            X = torch.randn(T, C, generator=g, device="cuda").half()
            _ops().h_accumulate(H[e], X, 0.0, 2.0 / (3 * C))  # one common scale
        H[2, C - 5, :] = 0
        H[2, :, C - 5] = 0
        A = torch.randn(E_MAX, R_MAX, C, generator=g, device="cuda") * 0.05
        noise = torch.randn(E_MAX, R_MAX, C, generator=g, device="cuda") * 0.05 * 0.02
        _made[C] = (A, noise, H)
    return _made[C]


def loop(A, H, B=None):
    ops = _ops()
    return torch.stack([ops.quad_form(A[e], H[e], None if B is None else B[e]) for e in range(A.shape[0])])


@pytest.mark.parametrize("C", CS)
def test_equals_the_per_expert_loop_bit_for_bit(C):
    ops = _ops()
    A32, noise, H = inputs(C)
    keep = H.clone()
    n = 0
    for R in RS:
        for E in ES:
            for da in DTYPES:
                A = A32[:E, :R].to(da).contiguous()
                Bs = [None, (A32 + noise)[:E, :R].to(da).contiguous(),
                      (A32 + noise)[:E, :R].to(DTYPES[(DTYPES.index(da) + 1) % 3]).contiguous()]
                for B in Bs:
                    got = ops.quad_form_experts(A, H[:E].contiguous(), B)
                    assert got.dtype == torch.float64 and tuple(got.shape) == (E,) and got.is_cuda
                    want = loop(A, H[:E], B)
                    assert torch.equal(_bits(got), _bits(want)), (R, E, da, None if B is None else B.dtype, got, want)
                    assert bool((got > 0).all())
                    n += 1
    assert torch.equal(H, keep)  # H is the caller's: not written
    print(f"C={C}: {n} grouped calls equal their loops")


@pytest.mark.parametrize("C", CS)
def test_never_routed_expert_and_dead_channel(C):
    """An all-zero H[e] is the identity (the squared norm of d); one zero diagonal entry reads as 1."""
    ops = _ops()
    A32, noise, H = inputs(C)
    assert float(H[1].abs().max()) == 0.0 and float(H[2, C - 5, C - 5]) == 0.0
    R = 130
    A, B = A32[:, :R].half().contiguous(), (A32 + noise)[:, :R].bfloat16().contiguous()
    eye = torch.eye(C, device="cuda")
    H1 = H.clone()
    H1[1] = eye
    H1[2, C - 5, C - 5] = 1
    for b in (None, B):
        got = ops.quad_form_experts(A, H, b)
        assert torch.equal(_bits(got), _bits(ops.quad_form_experts(A, H1, b)))
        assert torch.equal(_bits(got), _bits(loop(A, H, b)))
        d = A[1].float() - (b[1].float() if b is not None else 0)
        want = float(d.double().pow(2).sum())
        assert abs(got[1].item() - want) <= 2 * 2.0 ** -23 * want  # one fp32 rounding per product d * d, sums in fp64


@pytest.mark.parametrize("R", RS)
def test_both_halves_of_a_fused_tensor_are_read_in_place(R):
    """gate_up_proj [E, 2 R, C]: the gate half and the up half are views with expert stride 2 R C."""
    ops = _ops()
    C, E = 256, 5
    A32, noise, H = inputs(C)
    g = torch.Generator(device="cuda").manual_seed(R)
    for dt in DTYPES:
        fused = (torch.randn(E, 2 * R, C, generator=g, device="cuda") * 0.05).to(dt)
        comp = (fused.float() * 1.01).half()
        for half, chalf in ((fused[:, :R], comp[:, :R]), (fused[:, R:], comp[:, R:])):
            assert not half.is_contiguous() and half.stride(0) == 2 * R * C
            assert ops._qf_experts(half).data_ptr() == half.data_ptr()  # handed on, a_stride = 2 R C
            for b in (None, chalf):
                got = ops.quad_form_experts(half, H, b)
                want = loop(half.contiguous(), H, None if b is None else b.contiguous())
                assert torch.equal(_bits(got), _bits(want)), (R, dt)
    # an expert stride that is not a multiple of 16 bytes is copied by the op
    odd = torch.zeros(E, R * C + 4, dtype=torch.float16, device="cuda")
    view = odd[:, :R * C].view(E, R, C)
    odd[:, :R * C] = A32[:, :R].half().reshape(E, -1)
    assert ops._qf_experts(view).data_ptr() != view.data_ptr()
    assert torch.equal(_bits(ops.quad_form_experts(view, H)), _bits(loop(A32[:, :R].half(), H)))


def test_same_bits_twice_and_whatever_the_workspace_held():
    from gptq_gguf_toolkit_amd import _cabi
    ops = _ops()
    for C in CS:
        A32, noise, H = inputs(C)
        A, B = A32[:, :130].half().contiguous(), (A32 + noise)[:, :130].half().contiguous()
        first = ops.quad_form_experts(A, H, B)
        assert torch.equal(_bits(ops.quad_form_experts(A, H, B)), _bits(first))
        need = int(_cabi.lib().gq_quad_form_experts_workspace_bytes(E_MAX, 130, C))
        assert need == E_MAX * 2 * (C // 128) * 8
        for fill in (0xFF, 0x00):
            ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
            assert torch.equal(_bits(ops.quad_form_experts(A, H, B, ws=ws)), _bits(first))
        # the partials lie at ws[e * tiles + t], t the single call's tile number
        tiles = need // 8 // E_MAX
        ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        ops.quad_form_experts(A, H, B, ws=ws)
        for e in (0, E_MAX - 1):
            one = torch.zeros(tiles * 8, dtype=torch.uint8, device="cuda")
            ops.quad_form(A[e], H[e], B[e], ws=one)
            assert torch.equal(ws.view(torch.int64)[e * tiles:(e + 1) * tiles], one.view(torch.int64))


def test_refusals():
    from gptq_gguf_toolkit_amd import _cabi
    ops = _ops()
    A32, _, H = inputs(256)
    with pytest.raises(_cabi.GQError, match="C=192"):
        ops.quad_form_experts(torch.zeros(2, 4, 192, device="cuda"), torch.zeros(2, 192, 192, device="cuda"))
    with pytest.raises(_cabi.GQError, match="CPU"):
        ops.quad_form_experts(A32.cpu(), H)
    with pytest.raises(_cabi.GQError, match=r"\[E, R, C\]"):
        ops.quad_form_experts(A32[0], H)
    with pytest.raises(_cabi.GQError, match="H must be"):
        ops.quad_form_experts(A32, H[:3])
    with pytest.raises(_cabi.GQError):
        ops.quad_form_experts(A32, H, A32[:, :64])
    # a misaligned expert stride, handed to the library as it is: refused before anything is launched
    A = A32.half().contiguous()
    out, ws = torch.zeros(5, dtype=torch.float64, device="cuda"), torch.zeros(1024, dtype=torch.uint8, device="cuda")
    vp = ctypes.c_void_p
    with pytest.raises(_cabi.GQError, match="a_stride"):
        _cabi.check(_cabi.lib().gq_quad_form_experts(vp(A.data_ptr()), 1, 256, 130 * 256 - 4, vp(0), 0, 0, 0, vp(H.data_ptr()),
                                                     5, 129, 256, vp(out.data_ptr()), vp(ws.data_ptr()), 1024, vp(0)),
                    "gq_quad_form_experts")
    assert float(out.abs().max()) == 0.0
