"""Tensor-level entry points: torch CUDA(ROCm) tensors in, C-ABI calls out.

torch is plumbing here (device memory + the current HIP stream); every computation is
a kernel of libgptqgguf_hip.so.  All functions enqueue on torch's current stream and
return without synchronising.
"""
import ctypes
from typing import Optional, Sequence, Tuple

import torch

from . import _cabi
from ._cabi import F16, F32, BF16, Search, check, lib, type_info
from ._cabi import option_get, option_set, options  # noqa: F401  (library tuning / test switches)
from .gguf_writer import GGML_QUANT_SIZES, PACKED_TYPES  # (numpy-level host code: it imports neither this module nor the library)

_DT = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}


def _stream(t: torch.Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _cabi.GQError("gptq_gguf_toolkit_amd ops need GPU tensors (no CPU fallback); got a CPU tensor")


def _search(rmin=-1.0, rdelta=0.1, nstep=20, quant_scale="absmax", grid=100, maxshrink=0.8):
    """gq_search_t: make_k_quants' (rmin, rdelta, nstep) and make_quants' quant_scale ("absmax" | "mse", with the
    grid / maxshrink of quant_utils.py:164-191)."""
    mode = getattr(quant_scale, "value", quant_scale)
    if mode not in ("absmax", "mse"):
        raise ValueError(f"quant_scale must be 'absmax' or 'mse', got {quant_scale!r}")
    return ctypes.byref(Search(float(rmin), float(rdelta), int(nstep), int(mode == "mse"), int(grid), float(maxshrink)))


def _idt(q_type):
    return torch.int8 if type_info(q_type)["is_signed"] else torch.uint8


def _u8(t):
    return t.view(torch.uint8) if t.dtype != torch.uint8 else t


def _u16view(t):
    """fp16 tensor -> same storage seen as int16 (bit pattern carrier)."""
    return t.view(torch.int16) if t.dtype == torch.float16 else t


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def workspace_bytes(op: int, R=0, C=0, T=0, block_size=0) -> int:
    return int(lib().gq_workspace_bytes(op, R, C, T, block_size))


def h_accumulate(H: torch.Tensor, X: torch.Tensor, beta: float, alpha: float, ws: Optional[torch.Tensor] = None):
    """H = beta*H + alpha * X^T X in place.  X: [T, C] fp16/bf16/fp32 contiguous (or a list of equal [L, C] blocks)."""
    if isinstance(X, (list, tuple)):
        return h_accumulate_grouped([H], [X], [beta], [alpha], ws)[0]
    _need_cuda(H, X)
    assert H.dtype == torch.float32 and H.is_contiguous() and X.is_contiguous() and X.dim() == 2
    T, C = X.shape
    assert H.shape == (C, C)
    need = workspace_bytes(_cabi.WS_H_ACCUMULATE, 0, C, T)
    if ws is None or ws.numel() < need:
        ws = _ws(need, X.device)
    check(lib().gq_h_accumulate(_ptr(H), _ptr(X), _DT[X.dtype], T, C, beta, alpha, _ptr(ws), ws.numel(), _stream(X)),
          "gq_h_accumulate")
    return H


def h_accumulate_grouped(Hs, Xs, betas, alphas, ws: Optional[torch.Tensor] = None):
    """Up to 8 Hessians in one grid: Hs[i] = betas[i]*Hs[i] + alphas[i] * Xs[i]^T Xs[i].
    Xs[i] is a [T, C] tensor, or a LIST of [L, C] tensors (equal L, contiguous): the per-sample activation
    tensors of the forward hooks, read where they lie (gq_h_accumulate_segments)."""
    n = len(Hs)
    assert n == len(Xs) == len(betas) == len(alphas) and 1 <= n <= 8
    blocks = [list(X) if isinstance(X, (list, tuple)) else [X] for X in Xs]
    _need_cuda(*Hs, *[b for bl in blocks for b in bl])
    dt = blocks[0][0].dtype
    for H, bl in zip(Hs, blocks):
        assert H.dtype == torch.float32 and H.is_contiguous()
        for X in bl:
            assert X.is_contiguous() and X.dim() == 2 and X.dtype == dt and X.shape == bl[0].shape
        assert H.shape == (bl[0].shape[1], bl[0].shape[1])
    Ts = [len(bl) * bl[0].shape[0] for bl in blocks]
    need = sum(workspace_bytes(_cabi.WS_H_ACCUMULATE, 0, bl[0].shape[1], T) for bl, T in zip(blocks, Ts))
    if ws is None or ws.numel() < need:
        ws = _ws(need, blocks[0][0].device)
    vp = ctypes.c_void_p
    Hp = (vp * n)(*[H.data_ptr() for H in Hs])
    Cs = (ctypes.c_int64 * n)(*[bl[0].shape[1] for bl in blocks])
    bs = (ctypes.c_float * n)(*[float(b) for b in betas])
    as_ = (ctypes.c_float * n)(*[float(a) for a in alphas])
    if all(len(bl) == 1 for bl in blocks):
        Xp = (vp * n)(*[bl[0].data_ptr() for bl in blocks])
        Tc = (ctypes.c_int64 * n)(*Ts)
        check(lib().gq_h_accumulate_grouped(n, Hp, Xp, Tc, Cs, bs, as_, _DT[dt], _ptr(ws), ws.numel(),
                                            _stream(blocks[0][0])), "gq_h_accumulate_grouped")
        return Hs
    lists = [(vp * len(bl))(*[X.data_ptr() for X in bl]) for bl in blocks]
    Bp = (vp * n)(*[ctypes.cast(l, vp).value for l in lists])
    nb = (ctypes.c_int64 * n)(*[len(bl) for bl in blocks])
    bt = (ctypes.c_int64 * n)(*[bl[0].shape[0] for bl in blocks])
    check(lib().gq_h_accumulate_segments(n, Hp, Bp, nb, bt, Cs, bs, as_, _DT[dt], _ptr(ws), ws.numel(),
                                         _stream(blocks[0][0])), "gq_h_accumulate_segments")
    return Hs


def h_stage(buf: torch.Tensor, fill: int, x: torch.Tensor):
    """buf[fill : fill + T] = x  (x: [T, C] rows of activations, same dtype as the staging buffer `buf`)."""
    _need_cuda(buf, x)
    assert buf.is_contiguous() and buf.dtype == x.dtype and x.dim() == 2 and x.shape[1] == buf.shape[1]
    assert fill + x.shape[0] <= buf.shape[0]
    if not x.is_contiguous():
        x = x.contiguous()
    row = buf.shape[1] * buf.element_size()
    check(lib().gq_h_stage(ctypes.c_void_p(buf.data_ptr() + fill * row), _ptr(x), x.shape[0] * row, _stream(buf)),
          "gq_h_stage")


def h_stage_many(buf: torch.Tensor, fill: int, xs: Sequence[torch.Tensor]):
    """buf[fill : fill + sum T_k] = cat(xs) in ONE launch (xs: [T_k, C] contiguous blocks of the buffer's dtype, 16-byte
    aligned rows): the staging copies of a whole fold (gq_h_stage_many)."""
    _need_cuda(buf, *xs)
    row = buf.shape[1] * buf.element_size()
    total = sum(x.shape[0] for x in xs)
    assert buf.is_contiguous() and fill + total <= buf.shape[0] and row % 16 == 0
    assert all(x.dtype == buf.dtype and x.dim() == 2 and x.shape[1] == buf.shape[1] and x.is_contiguous() for x in xs)
    n = len(xs)
    srcs = (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
    nb = (ctypes.c_int64 * n)(*[x.shape[0] * row for x in xs])
    ws = _ws((2 * n + 1) * 8 + 512, buf.device)
    check(lib().gq_h_stage_many(ctypes.c_void_p(buf.data_ptr() + fill * row), srcs, nb, n, _ptr(ws), ws.numel(), _stream(buf)),
          "gq_h_stage_many")


def h_prepare(H: torch.Tensor, W: torch.Tensor, rel_damp: float, want_flags: bool = False, obq_order: bool = False):
    """In-place dead-channel fix / masking / damping of (H, W); returns (U, not_invertible[int32 tensor])
    (+ col_flags uint8[2*C] if want_flags: the dead / zero-column sets U depends on).  obq_order: damping before
    the zero-column mask (EvoPress FastOBQ, evopress/src/fast_obq.py:133-141, 221-228)."""
    _need_cuda(H, W)
    assert H.dtype == torch.float32 and W.dtype == torch.float32 and H.is_contiguous() and W.is_contiguous()
    R, C = W.shape
    U = torch.empty_like(H)
    flag = torch.empty(1, dtype=torch.int32, device=H.device)  # cleared by the call (hipMemsetAsync on its stream)
    cf = torch.empty(2 * C, dtype=torch.uint8, device=H.device) if want_flags else None
    ws = _ws(workspace_bytes(_cabi.WS_H_PREPARE, R, C), H.device)
    fn = lib().gq_obq_h_prepare if obq_order else lib().gq_h_prepare
    check(fn(_ptr(H), _ptr(W), R, C, rel_damp, _ptr(U), _ptr(flag), _ptr(cf), _ptr(ws), ws.numel(), _stream(H)),
          "gq_obq_h_prepare" if obq_order else "gq_h_prepare")
    return (U, flag, cf) if want_flags else (U, flag)


def w_prepare(col_flags: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """Follower of a shared Hessian: zero this W's dead columns; returns mismatch[int32 tensor]
    (0 => the leader's U is this Linear's U)."""
    _need_cuda(col_flags, W)
    assert W.dtype == torch.float32 and W.is_contiguous() and col_flags.numel() == 2 * W.shape[1]
    mm = torch.empty(1, dtype=torch.int32, device=W.device)  # cleared by the call
    check(lib().gq_w_prepare(_ptr(col_flags), _ptr(W), W.shape[0], W.shape[1], _ptr(mm), _stream(W)), "gq_w_prepare")
    return mm


def h_pack_upper(H: torch.Tensor) -> torch.Tensor:
    """The 128x128 tiles of H on and above the diagonal as one contiguous fp32 buffer (the all-reduce payload)."""
    _need_cuda(H)
    C = H.shape[0]
    assert H.dtype == torch.float32 and H.is_contiguous() and H.shape == (C, C) and C % 128 == 0
    nt = C // 128
    buf = torch.empty(nt * (nt + 1) // 2, 128, 128, dtype=torch.float32, device=H.device)
    check(lib().gq_h_pack_upper(_ptr(H), C, _ptr(buf), _stream(H)), "gq_h_pack_upper")
    return buf


def h_unpack_upper(buf: torch.Tensor, H: torch.Tensor) -> torch.Tensor:
    """Inverse of h_pack_upper: writes the tiles back into H and mirrors them below the diagonal."""
    _need_cuda(buf, H)
    C = H.shape[0]
    assert H.dtype == torch.float32 and H.is_contiguous() and buf.dtype == torch.float32 and buf.is_contiguous()
    check(lib().gq_h_unpack_upper(_ptr(buf), C, _ptr(H), _stream(H)), "gq_h_unpack_upper")
    return H


def scale_search(x: torch.Tensor, q_type: int, rmin=-1.0, rdelta=0.1, nstep=20, **mq):
    """get_scale_and_zero on x[rows,256] (row stride free).  Returns (d f16[rows], s[rows,ng], dmin f16[rows], m)."""
    _need_cuda(x)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == 256 and x.stride(1) == 1
    rows = x.shape[0]
    ng = 256 // type_info(q_type)["group"]
    dev = x.device
    d = torch.empty(rows, dtype=torch.float16, device=dev)
    dmin = torch.empty(rows, dtype=torch.float16, device=dev)
    s = torch.empty(rows, ng, dtype=torch.uint8, device=dev)
    m = torch.empty(rows, ng, dtype=torch.uint8, device=dev)
    check(lib().gq_scale_search(_ptr(x), rows, x.stride(0), int(q_type), _search(rmin, rdelta, nstep, **mq), _ptr(d), 1,
                                _ptr(s), ng, _ptr(dmin), 1, _ptr(m), ng, _stream(x)), "gq_scale_search")
    t = _idt(q_type)
    return d, s.view(t), dmin, m.view(t)


def _alloc_outs(R, C, q_type, dev):
    G = type_info(q_type)["group"]
    return (torch.empty(R, C, dtype=torch.uint8, device=dev), torch.empty(R, C // 256, dtype=torch.float16, device=dev),
            torch.empty(R, C // G, dtype=torch.uint8, device=dev),
            torch.empty(R, C // 256, dtype=torch.float16, device=dev),
            torch.empty(R, C // G, dtype=torch.uint8, device=dev))


def _walk_ws(ws: Optional[torch.Tensor], R, C, bs, device) -> torch.Tensor:
    """The column walk's workspace: the caller's when it is at least the needed size, else a fresh one."""
    need = workspace_bytes(_cabi.WS_GPTQ_QUANTIZE, R, C, 0, bs)
    return ws if ws is not None and ws.numel() >= need else _ws(need, device)


def _kquant_outs(q_type, q, d, s, dmin, m):
    t = _idt(q_type)
    return q.view(t), d, s.view(t), dmin, m.view(t)


_side_streams = {}


def _streams(device, n):
    pool = _side_streams.setdefault(device, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device))
    return pool[:n]


def gptq_quantize(W: torch.Tensor, U: torch.Tensor, q_type: int, block_size=128, static_groups=False, rmin=-1.0,
                  rdelta=0.1, nstep=20, ws: Optional[torch.Tensor] = None, row_chunks: Optional[int] = None,
                  row_ends: Optional[Sequence[int]] = None, panel_researches: Optional[torch.Tensor] = None, **mq):
    """GPTQ.step body.  W (fp32, contiguous) is updated IN PLACE to the dequantized matrix.
    Returns (qweight, d, s, dmin, m).

    `panel_researches` (gq_gptq_quantize_slice): W is a ROW SLICE of a matrix several ranks quantize together; the int32
    device tensor receives the number of panel-wide re-searches of the slice's scale searches (0: the slice's rows equal
    the whole matrix's rows bit for bit -- quant_utils.py:250-252 is the one place the reference looks across all rows).

    `row_ends` (gq_gptq_quantize_stacked): W holds several Linears that share U, one under the other -- matrix k is rows
    [row_ends[k-1], row_ends[k]), multiples of 64, the last one == R.  One walk over the columns instead of one per
    Linear; every output row equals the separate calls bit for bit (the scale search's panel-wide `continue`,
    quant_utils.py:250-252, is evaluated per stacked matrix).

    Rows of W are independent given U (gptq.py:222-270 never mixes rows), so a tall matrix is cut into
    `row_chunks` contiguous row ranges, each a separate gq_gptq_quantize call on its own HIP stream: the
    latency-bound column-loop kernel of one chunk overlaps with the trailing-update GEMM of another.
    Results are identical to one call.  Default 1 (what BlockSchedule uses): every extra chunk multiplies the
    launch count; measured no gain inside a block's four-chain schedule."""
    _need_cuda(W, U)
    assert W.dtype == torch.float32 and U.dtype == torch.float32 and W.is_contiguous() and U.is_contiguous()
    R, C = W.shape
    q, d, s, dmin, m = _alloc_outs(R, C, q_type, W.device)
    bs = int(block_size or 0)
    if row_chunks is None:
        row_chunks = 1
    if row_chunks > 1 and (R % (64 * row_chunks) or ws is not None):
        row_chunks = 1

    def one(r0, r1, wsbuf, entry="gq_gptq_quantize", extra=()):
        """rows [r0, r1) through one entry point: all three take `extra` between the outputs and the workspace"""
        n = r1 - r0
        wsbuf = _walk_ws(wsbuf, n, C, bs, W.device)
        check(getattr(lib(), entry)(_ptr(W[r0:r1]), _ptr(U), n, C, int(q_type), bs, int(bool(static_groups)),
                                    _search(rmin, rdelta, nstep, **mq), _ptr(q[r0:r1]), _ptr(d[r0:r1]), _ptr(s[r0:r1]),
                                    _ptr(dmin[r0:r1]), _ptr(m[r0:r1]), *extra, _ptr(wsbuf), wsbuf.numel(), _stream(W)), entry)
        return wsbuf

    if row_ends is not None and len(row_ends) > 1:
        ends = (ctypes.c_int64 * len(row_ends))(*[int(e) for e in row_ends])
        one(0, R, ws, "gq_gptq_quantize_stacked", (ends, len(row_ends)))
    elif panel_researches is not None:
        assert panel_researches.dtype == torch.int32 and panel_researches.is_cuda and panel_researches.numel() >= 1
        one(0, R, ws, "gq_gptq_quantize_slice", (_ptr(panel_researches),))
    elif row_chunks == 1:
        one(0, R, ws)
    else:
        cur = torch.cuda.current_stream(W.device)
        fork = torch.cuda.Event()
        fork.record(cur)
        step = R // row_chunks
        keep = []
        for k, st in enumerate(_streams(W.device, row_chunks)):
            st.wait_event(fork)
            with torch.cuda.stream(st):
                keep.append(one(k * step, (k + 1) * step, None))
            ev = torch.cuda.Event()
            ev.record(st)
            cur.wait_event(ev)
        for b in keep:  # scratch was allocated on side streams; it is dead once `cur` has passed the joins
            b.record_stream(cur)
    return _kquant_outs(q_type, q, d, s, dmin, m)


BANDS_MAX = _cabi.BANDS_MAX
_K_GROUP = {10: 16, 11: 16, 12: 32, 13: 32, 14: 16}   # group size of Q2_K .. Q6_K (quant_utils.py:19-26)
_K_SIGNED = {10: False, 11: True, 12: False, 13: False, 14: True}


def band_layout(bands: Sequence[Tuple[int, int]], C: int):
    """Pure: where the bands of a gq_gptq_quantize_bands call lie.  `bands` is the call's table, (row_end, q_type) per band,
    ascending.  -> [(row0, row1, q_type, group, sm_off)] per band and the total bytes of s (and of m): band k's
    [rows_k, C / group_k] array starts at byte sm_off = sum_{j<k} rows_j * C / group_j.  Raises ValueError for a table the
    library would refuse (so that a caller's mistake shows before any allocation)."""
    if not 1 <= len(bands) <= BANDS_MAX:
        raise ValueError(f"{len(bands)} bands (1..{BANDS_MAX})")
    out, r0, off = [], 0, 0
    for k, (r1, t) in enumerate(bands):
        r1, t = int(r1), int(t)
        if t not in _K_GROUP:
            raise ValueError(f"band {k} has unknown q_type {t}")
        if r1 % 64 or r1 <= r0:
            raise ValueError(f"band {k} ends at row {r1} (ascending multiples of 64)")
        g = _K_GROUP[t]
        out.append((r0, r1, t, g, off))
        off += (r1 - r0) * (C // g)
        r0 = r1
    return out, off


def gptq_quantize_bands(W: torch.Tensor, U: torch.Tensor, bands: Sequence[Tuple[int, int]], block_size=128, rmin=-1.0,
                        rdelta=0.1, nstep=20, ws: Optional[torch.Tensor] = None, return_stacked: bool = False, **mq):
    """The column walk of gptq_quantize over row bands of DIFFERENT K-quant types that share U (gq_gptq_quantize_bands):
    W (fp32, contiguous) holds several working copies one under the other, band k = rows [row_end[k-1], row_end[k]) is
    quantized to q_type[k]; `bands` = [(row_end, q_type)], row ends ascending multiples of 64, the last one == R.  One
    walk over the columns for all bands; every band's rows equal gptq_quantize on those rows alone with that type, bit
    for bit.  W is updated IN PLACE.  Returns one (qweight, d, s, dmin, m) per band: views into the stacked outputs; with
    `return_stacked` also the stacked outputs themselves, (views, (qweight, d, s, dmin, m)), as pack_bands takes them."""
    _need_cuda(W, U)
    assert W.dtype == torch.float32 and U.dtype == torch.float32 and W.is_contiguous() and U.is_contiguous()
    R, C = W.shape
    n = len(bands)
    tbl = (_cabi.Band * max(n, 1))(*[_cabi.Band(int(e), int(t)) for e, t in bands])
    dev = W.device
    q = torch.empty(R, C, dtype=torch.uint8, device=dev)
    d = torch.empty(R, C // 256, dtype=torch.float16, device=dev)
    dmin = torch.empty(R, C // 256, dtype=torch.float16, device=dev)
    s = torch.empty(R * (C // 16), dtype=torch.uint8, device=dev)  # G >= 16: room for any table
    m = torch.empty(R * (C // 16), dtype=torch.uint8, device=dev)
    bs = int(block_size or 0)
    if ws is None:  # a caller's own workspace goes to the library as it is: a short one is the library's to refuse
        ws = _walk_ws(None, R, C, bs, dev)
    check(lib().gq_gptq_quantize_bands(_ptr(W), _ptr(U), R, C, tbl, n, bs, _search(rmin, rdelta, nstep, **mq), _ptr(q),
                                       _ptr(d), _ptr(s), _ptr(dmin), _ptr(m), _ptr(ws), ws.numel(), _stream(W)),
          "gq_gptq_quantize_bands")
    lay, _ = band_layout(bands, C)
    out = []
    for r0, r1, t, g, off in lay:
        it = torch.int8 if _K_SIGNED[t] else torch.uint8
        nb = (r1 - r0) * (C // g)
        out.append((q[r0:r1].view(it), d[r0:r1], s[off:off + nb].view(r1 - r0, C // g).view(it), dmin[r0:r1],
                    m[off:off + nb].view(r1 - r0, C // g).view(it)))
    return (out, (q, d, s, dmin, m)) if return_stacked else out


# ---- the bands of a walk as GGUF block bytes (gq_pack_bands) ----
def pack_bands_plan(bands: Sequence[Tuple[int, int]], C: int):
    """Pure: what a gq_pack_bands call over `bands` (the table of band_layout) writes.  -> [(row0, row1, q_type, row_bytes,
    nbytes, off)] per band and the total: band k packs to [rows_k, row_bytes] = nbytes bytes, and `off` is where it lies when
    all bands share one buffer (the prefix sum: every nbytes is a multiple of 64 * type_size, so every band starts 16-byte
    aligned).  Raises ValueError for what the library would refuse."""
    C = int(C)
    if C <= 0 or C % 256:
        raise ValueError(f"C={C} (a positive multiple of 256)")
    lay, _ = band_layout(bands, C)
    out, off = [], 0
    for r0, r1, t, _, _ in lay:
        row_bytes = C // 256 * GGML_QUANT_SIZES[t][1]
        out.append((r0, r1, t, row_bytes, (r1 - r0) * row_bytes, off))
        off += (r1 - r0) * row_bytes
    return out, off


def _stacked_of(results, lay, C):
    """The stacked (q, d, s, dmin, m) buffers behind per-band views (what gptq_quantize_bands returns), as raw pointers."""
    es = {0: 1, 1: 2, 2: 1, 3: 2, 4: 1}
    base = [results[0][i].data_ptr() for i in range(5)]
    for (r0, r1, t, g, off), res in zip(lay, results):
        want = (r0 * C, r0 * (C // 256) * 2, off, r0 * (C // 256) * 2, off)
        for i in range(5):
            if not res[i].is_contiguous() or res[i].data_ptr() != base[i] + want[i] or \
                    res[i].numel() * es[i] != (r1 - r0) * (C, C // 256 * 2, C // g, C // 256 * 2, C // g)[i]:
                raise _cabi.GQError("pack_bands: the per-band results are not views into one set of stacked buffers in "
                                    "band order (pass gptq_quantize_bands' results, or the stacked tensors themselves)")
    return base


def pack_bands(results, bands: Sequence[Tuple[int, int]], outs: Optional[Sequence[torch.Tensor]] = None,
               row_srcs: Optional[Sequence[Optional[torch.Tensor]]] = None):
    """The outputs of ONE gptq_quantize_bands call as GGUF block bytes, every band into a buffer of its own, in one launch
    (gq_pack_bands).  `results`: that call's per-band views, or its stacked (qweight [R, C], d, s, dmin, m) tensors
    (return_stacked); `bands`: its table.  outs[k]: contiguous uint8 of pack_bands_plan's nbytes, 16-byte aligned (None:
    allocated here, one buffer cut by the plan's offsets).  row_srcs[k]: None or int32 [rows_k] on the device, output row r
    of band k is packed from band row row_srcs[k][r]; indices are trusted.  Band k's bytes equal
    pack(q_type_k, *[t[row_srcs[k]] for t in band k]) bit for bit.  -> the outs as [rows_k, row_bytes] views.  Inputs are
    not modified; no host read."""
    n = len(bands)
    stacked = len(results) == 5 and all(torch.is_tensor(t) for t in results)
    q0 = results[0] if stacked else results[0][0]
    _need_cuda(q0)
    dev = q0.device
    C = int(q0.shape[1])
    plan, total = pack_bands_plan(bands, C)
    lay, _ = band_layout(bands, C)
    R = plan[-1][1]
    if stacked:
        q, d, s, dmin, m = results
        _need_cuda(q, d, s, dmin, m)
        if not all(t.is_contiguous() for t in results) or tuple(q.shape) != (R, C) or d.numel() != R * (C // 256) \
                or dmin.numel() != d.numel() or s.numel() < lay[-1][4] + (R - lay[-1][0]) * (C // lay[-1][3]) or m.numel() < s.numel():
            raise _cabi.GQError(f"pack_bands: stacked inputs do not fit the table (R={R}, C={C})")
        base = [t.data_ptr() for t in results]
    else:
        if len(results) != n:
            raise _cabi.GQError(f"pack_bands: {len(results)} results for {n} bands")
        _need_cuda(*[t for res in results for t in res])
        base = _stacked_of(results, lay, C)
    if outs is None:
        buf = torch.empty(total, dtype=torch.uint8, device=dev)
        outs = [buf[off:off + nb] for _, _, _, _, nb, off in plan]
    if len(outs) != n or (row_srcs is not None and len(row_srcs) != n):
        raise _cabi.GQError(f"pack_bands: outs / row_srcs must have one entry per band ({n})")
    vp = ctypes.c_void_p
    op, rp = (vp * n)(), (vp * n)()
    for k, (r0, r1, t, row_bytes, nb, _) in enumerate(plan):
        o = outs[k]
        _need_cuda(o)
        if o.dtype != torch.uint8 or not o.is_contiguous() or o.numel() != nb or o.device != dev:
            raise _cabi.GQError(f"pack_bands: outs[{k}] must be a contiguous uint8 tensor of {nb} bytes on {dev}; got {o.dtype} "
                                f"{tuple(o.shape)}")
        op[k] = o.data_ptr()
        rs = row_srcs[k] if row_srcs is not None else None
        if rs is not None:
            _need_cuda(rs)
            if rs.dtype != torch.int32 or rs.numel() != r1 - r0 or not rs.is_contiguous() or rs.device != dev:
                raise _cabi.GQError(f"pack_bands: row_srcs[{k}] must be a contiguous int32 [{r1 - r0}] tensor on {dev}")
            rp[k] = rs.data_ptr()
    tbl = (_cabi.Band * n)(*[_cabi.Band(int(e), int(t)) for e, t in bands])
    check(lib().gq_pack_bands(vp(base[0]), vp(base[1]), vp(base[2]), vp(base[3]), vp(base[4]), R, C, tbl, n, op, rp,
                              _stream(q0)), "gq_pack_bands")
    return [o.view(r1 - r0, row_bytes) for o, (r0, r1, _, row_bytes, _, _) in zip(outs, plan)]


def uses_helper_stream(R: int, C: int, block_size) -> bool:
    """Will the column loop of an R x C matrix run its far updates on the library's helper stream (gq_gptq_uses_helper_stream)?"""
    return bool(lib().gq_gptq_uses_helper_stream(int(R), int(C), int(block_size or 0)))


def far_helper_enable(on: bool) -> bool:
    """Allow / forbid the library's helper stream for the column loops enqueued from now on; returns the previous setting."""
    return bool(lib().gq_far_helper_enable(int(bool(on))))


def gptq_quantize_perm(W: torch.Tensor, U: torch.Tensor, q_type: int, perm: torch.Tensor, d, s, dmin, m, block_size=128,
                       ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GPTQ.step body with act_order (gptq.py:208-216, 233-235).  W (fp32) and U are already permuted by `perm`
    (int32 [C], original column of each position); (d, s, dmin, m) are the static scales of the ORIGINAL column
    groups.  W becomes the dequantized matrix (permuted); returns qweight in permuted positions."""
    _need_cuda(W, U, perm, d, s, dmin, m)
    assert W.dtype == torch.float32 and U.dtype == torch.float32 and W.is_contiguous() and U.is_contiguous()
    assert perm.dtype == torch.int32 and perm.is_contiguous() and perm.numel() == W.shape[1]
    R, C = W.shape
    q = torch.empty(R, C, dtype=torch.uint8, device=W.device)
    bs = int(block_size or 0)
    ws = _walk_ws(ws, R, C, bs, W.device)
    check(lib().gq_gptq_quantize_perm(_ptr(W), _ptr(U), R, C, int(q_type), bs, _ptr(perm), _ptr(d.contiguous()),
                                      _ptr(s.contiguous()), _ptr(dmin.contiguous()), _ptr(m.contiguous()), _ptr(q),
                                      _ptr(ws), ws.numel(), _stream(W)), "gq_gptq_quantize_perm")
    return q.view(_idt(q_type))


def obq_quantize(W: torch.Tensor, U: torch.Tensor, bits: int, group_size: int = 0, sym: bool = False, block_size=128,
                 ws: Optional[torch.Tensor] = None):
    """EvoPress FastOBQ.step for one bit width (evopress/src/fast_obq.py:146-200).  W (fp32, contiguous) becomes
    the dequantized matrix.  Returns (qweight u8 [R, C], scale f32 [R, C/G], zero f32 [R, C/G])."""
    _need_cuda(W, U)
    assert W.dtype == torch.float32 and U.dtype == torch.float32 and W.is_contiguous() and U.is_contiguous()
    R, C = W.shape
    ng = C // group_size if group_size else 1
    q = torch.empty(R, C, dtype=torch.uint8, device=W.device)
    scale = torch.empty(R, ng, dtype=torch.float32, device=W.device)
    zero = torch.empty(R, ng, dtype=torch.float32, device=W.device)
    bs = int(block_size or 0)
    ws = _walk_ws(ws, R, C, bs, W.device)
    check(lib().gq_obq_quantize(_ptr(W), _ptr(U), R, C, int(bits), int(group_size or 0), int(bool(sym)), bs, _ptr(q),
                                _ptr(scale), _ptr(zero), _ptr(ws), ws.numel(), _stream(W)), "gq_obq_quantize")
    return q, scale, zero


def rtn_quantize(W: torch.Tensor, q_type: int, rmin=-1.0, rdelta=0.1, nstep=20, **mq):
    _need_cuda(W)
    assert W.is_contiguous() and W.dim() == 2 and W.dtype in _DT
    R, C = W.shape
    q, d, s, dmin, m = _alloc_outs(R, C, q_type, W.device)
    check(lib().gq_rtn_quantize(_ptr(W), _DT[W.dtype], R, C, int(q_type), _search(rmin, rdelta, nstep, **mq), _ptr(q),
                                _ptr(d), _ptr(s), _ptr(dmin), _ptr(m), _stream(W)), "gq_rtn_quantize")
    t = _idt(q_type)
    return q.view(t), d, s.view(t), dmin, m.view(t)


def dequantize(q_type: int, q, d, s, dmin, m, out_dtype=torch.float32) -> torch.Tensor:
    _need_cuda(q, d, s, dmin, m)
    R, C = q.shape
    out = torch.empty(R, C, dtype=out_dtype, device=q.device)
    check(lib().gq_dequantize(int(q_type), _ptr(q.contiguous()), _ptr(d.contiguous()), _ptr(s.contiguous()),
                              _ptr(dmin.contiguous()), _ptr(m.contiguous()), R, C, _ptr(out), _DT[out_dtype],
                              _stream(q)), "gq_dequantize")
    return out


def pack(q_type: int, q, d, s, dmin=None, m=None) -> torch.Tensor:
    """-> uint8 [R, C/256*type_size] on the device.  Inputs are not modified."""
    _need_cuda(q, d, s, dmin, m)
    R, C = q.shape
    ts = type_info(q_type)["type_size"]
    out = torch.empty(R, C // 256 * ts, dtype=torch.uint8, device=q.device)
    check(lib().gq_pack(int(q_type), _ptr(q.contiguous()), _ptr(d.contiguous()), _ptr(s.contiguous()),
                        _ptr(dmin.contiguous() if dmin is not None else None),
                        _ptr(m.contiguous() if m is not None else None), R, C, _ptr(out), _stream(q)), "gq_pack")
    return out


def unpack(q_type: int, blocks: torch.Tensor):
    """Inverse of pack: uint8 [R, C/256*type_size] -> (q [R, C], d f16 [R, C/256], s [R, C/G], dmin, m) with the dtypes of the
    quantize entry points (int8 views of q / s / m for Q3_K / Q6_K, whose dmin / m come back as zeros)."""
    _need_cuda(blocks)
    ts = type_info(q_type)["type_size"]
    assert blocks.dtype == torch.uint8 and blocks.dim() == 2 and blocks.shape[1] % ts == 0
    blocks = blocks.contiguous()
    R, C = blocks.shape[0], blocks.shape[1] // ts * 256
    q, d, s, dmin, m = _alloc_outs(R, C, q_type, blocks.device)
    check(lib().gq_unpack(int(q_type), _ptr(blocks), R, C, _ptr(q), _ptr(d), _ptr(s), _ptr(dmin), _ptr(m), _stream(blocks)),
          "gq_unpack")
    t = _idt(q_type)
    return q.view(t), d, s.view(t), dmin, m.view(t)


def block_geometry(q_type: int) -> Tuple[int, int]:
    """(values per block, bytes per block) of a type gq_dequantize_blocks / gq_level_switch decode, from the one table
    gguf_writer.GGML_QUANT_SIZES: the K-quants' 256-value blocks, Q8_0's 32 values in 34 bytes, IQ4_NL's 32 in 18 and IQ4_XS's
    256 in 136.  Any other type is refused as the library refuses it."""
    if int(q_type) not in PACKED_TYPES:
        raise _cabi.GQError(f"block_geometry: unknown q_type {int(q_type)} (a K-quant, Q8_0, IQ4_NL or IQ4_XS)")
    return GGML_QUANT_SIZES[int(q_type)]


def dequantize_blocks(q_type: int, blocks: torch.Tensor, out_dtype=torch.float32,
                      row_src: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Packed blocks uint8 [R, C/block*type_size] -> weights [R, C] in one pass (gq_dequantize_blocks): for a K-quant bit
    for bit dequantize(*unpack(blocks)), for Q8_0 (blocks of 32 values in 34 bytes) `d.float() * q.float()` and one cast.
    row_src (int32 [R] on the device): out[r] = decode(blocks[row_src[r]]); every index must lie in [0, R) -- the kernel
    does not check."""
    _need_cuda(blocks, row_src)
    bs, ts = block_geometry(q_type)
    if blocks.dtype != torch.uint8 or blocks.dim() != 2 or blocks.shape[1] % ts:
        raise _cabi.GQError(f"dequantize_blocks: packed blocks of q_type {int(q_type)} must be uint8 [R, C/{bs}*{ts}]; got "
                            f"{blocks.dtype} {tuple(blocks.shape)}")
    blocks = blocks.contiguous()
    R, C = blocks.shape[0], blocks.shape[1] // ts * bs
    if row_src is not None:
        assert row_src.dtype == torch.int32 and row_src.numel() == R and row_src.device == blocks.device
        row_src = row_src.contiguous()
    out = torch.empty(R, C, dtype=out_dtype, device=blocks.device)
    check(lib().gq_dequantize_blocks(int(q_type), _ptr(blocks), R, C, _ptr(row_src), _ptr(out), _DT[out_dtype],
                                     _stream(blocks)), "gq_dequantize_blocks")
    return out


def quantize_q8_0(x: torch.Tensor, row_src: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[R, C] fp32 / fp16 / bf16 on the device -> Q8_0 blocks uint8 [R, C/32*34] (gq_quantize_q8_0): bit for bit
    gguf_writer.quantize_q8_0 of x widened to fp32.  row_src (int32 [R] on the device): out[r] = encode(x[row_src[r]]);
    every index must lie in [0, R) -- the kernel does not check."""
    _need_cuda(x, row_src)
    if x.dim() != 2 or x.dtype not in _DT or x.shape[1] % 32 or x.shape[0] < 1 or x.shape[1] < 32:
        raise _cabi.GQError(f"quantize_q8_0: x must be a [R, C] fp32 / fp16 / bf16 tensor with C % 32 == 0; got {x.dtype} "
                            f"{tuple(x.shape)}")
    x = x.contiguous()
    R, C = x.shape
    if row_src is not None:
        if row_src.dtype != torch.int32 or row_src.numel() != R or row_src.device != x.device:
            raise _cabi.GQError(f"quantize_q8_0: row_src must be an int32 [{R}] tensor on {x.device}")
        row_src = row_src.contiguous()
    out = torch.empty(R, C // 32 * 34, dtype=torch.uint8, device=x.device)
    check(lib().gq_quantize_q8_0(_ptr(x), _DT[x.dtype], R, C, _ptr(row_src), _ptr(out), _stream(x)), "gq_quantize_q8_0")
    return out


def quantize_iq4(x: torch.Tensor, q_type: int, importance: Optional[torch.Tensor] = None,
                 row_src: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[R, C] fp32 / fp16 / bf16 on the device -> IQ4_NL (q_type 20, C % 32 == 0) blocks uint8 [R, C/32*18] or IQ4_XS (23,
    C % 256 == 0) blocks uint8 [R, C/256*136] (gq_quantize_iq4, include/gptq_gguf_iq4_encode.h): byte for byte
    gguf_writer.quantize_iq4 of x widened to fp32.  importance: None, or fp32 [C] on x's device, finite and >= 0, one weight
    per column (the diagonal of the calibration Hessian is one).  row_src (int32 [R] on the device): out[r] =
    encode(x[row_src[r]]); every index must lie in [0, R) -- the kernel does not check.  out: None, or a contiguous uint8
    tensor of exactly the result's bytes on x's device, 16-byte aligned (a slot of a stacked buffer), written in place and
    returned as the [R, row bytes] view."""
    _need_cuda(x, row_src, out)
    if int(q_type) not in (_cabi.IQ4_NL, _cabi.IQ4_XS):
        raise _cabi.GQError(f"quantize_iq4: q_type {int(q_type)} is neither IQ4_NL ({_cabi.IQ4_NL}) nor IQ4_XS ({_cabi.IQ4_XS})")
    bs, ts = GGML_QUANT_SIZES[int(q_type)]
    if x.dim() != 2 or x.dtype not in _DT or x.shape[1] % bs or x.shape[0] < 1 or x.shape[1] < bs:
        raise _cabi.GQError(f"quantize_iq4: x must be a [R, C] fp32 / fp16 / bf16 tensor with C % {bs} == 0; got {x.dtype} "
                            f"{tuple(x.shape)}")
    R, C = x.shape
    if importance is not None:
        if importance.dtype != torch.float32 or importance.dim() != 1 or importance.numel() != C or importance.device != x.device:
            raise _cabi.GQError(f"quantize_iq4: importance must be an fp32 [{C}] tensor on {x.device}; got {importance.dtype} "
                                f"{tuple(importance.shape)} on {importance.device}")
    if row_src is not None:
        if row_src.dtype != torch.int32 or row_src.numel() != R or row_src.device != x.device:
            raise _cabi.GQError(f"quantize_iq4: row_src must be an int32 [{R}] tensor on {x.device}")
        row_src = row_src.contiguous()
    if x.is_contiguous() and x.data_ptr() % 16:
        raise _cabi.GQError("quantize_iq4: x must be 16-byte aligned")
    x = x.contiguous()
    if importance is not None:
        importance = importance.contiguous()
        if importance.data_ptr() % 16:  # (a view into a larger buffer)
            importance = importance.clone()
    if out is None:
        out = torch.empty(R, C // bs * ts, dtype=torch.uint8, device=x.device)
    else:
        if out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != R * (C // bs * ts) or out.device != x.device \
                or out.data_ptr() % 16:
            raise _cabi.GQError(f"quantize_iq4: out must be a contiguous, 16-byte aligned uint8 tensor of {R * (C // bs * ts)} "
                                f"bytes on {x.device}; got {out.dtype} {tuple(out.shape)}")
        out = out.view(R, C // bs * ts)
    check(lib().gq_quantize_iq4(_ptr(x), _DT[x.dtype], R, C, int(q_type), _ptr(importance), _ptr(row_src), _ptr(out), _stream(x)),
          "gq_quantize_iq4")
    return out


def _iq4_type(what: str, q_type: int) -> bool:
    if int(q_type) not in (_cabi.IQ4_NL, _cabi.IQ4_XS):
        raise _cabi.GQError(f"{what}: q_type {int(q_type)} is neither IQ4_NL ({_cabi.IQ4_NL}) nor IQ4_XS ({_cabi.IQ4_XS})")
    return int(q_type) == _cabi.IQ4_XS


def gptq_quantize_iq4(W: torch.Tensor, U: torch.Tensor, q_type: int, block_size=128, importance: Optional[torch.Tensor] = None,
                      ws: Optional[torch.Tensor] = None):
    """GPTQ's column walk on the IQ4_XS / IQ4_NL grid (gq_gptq_quantize_iq4, include/gptq_gguf_iq4_gptq.h): the scales of a
    256-column group come from the encoder's scale search on the error-compensated weights when the walk reaches the group,
    every rounding error goes into later columns through U.  W (fp32 [R, C], C % 256 == 0, contiguous) becomes exactly what
    dequantize_blocks makes of pack_iq4 of the outputs.  importance: None or fp32 [C] as for quantize_iq4.
    Returns (qweight u8 [R, C] codes 0..15, d f16 [R, C/256] (IQ4_XS) / [R, C/32] (IQ4_NL), ls u8 [R, C/32] (IQ4_XS) / None,
    step f32 [R, C/32])."""
    _need_cuda(W, U, importance)
    xs = _iq4_type("gptq_quantize_iq4", q_type)
    assert W.dtype == torch.float32 and U.dtype == torch.float32 and W.is_contiguous() and U.is_contiguous() and W.dim() == 2
    R, C = W.shape
    if importance is not None:
        if importance.dtype != torch.float32 or importance.dim() != 1 or importance.numel() != C or importance.device != W.device:
            raise _cabi.GQError(f"gptq_quantize_iq4: importance must be an fp32 [{C}] tensor on {W.device}; got {importance.dtype} "
                                f"{tuple(importance.shape)} on {importance.device}")
        importance = importance.contiguous()
        if importance.data_ptr() % 16:  # (a view into a larger buffer)
            importance = importance.clone()
    nb = max(C // 32, 1)
    q = torch.empty(R, C, dtype=torch.uint8, device=W.device)
    d = torch.empty(R, max(C // 256, 1) if xs else nb, dtype=torch.float16, device=W.device)
    ls = torch.empty(R, nb, dtype=torch.uint8, device=W.device) if xs else None
    step = torch.empty(R, nb, dtype=torch.float32, device=W.device)
    istep = torch.empty(R, nb, dtype=torch.float32, device=W.device)
    bs = int(block_size or 0)
    ws = _walk_ws(ws, R, C, bs, W.device)
    check(lib().gq_gptq_quantize_iq4(_ptr(W), _ptr(U), R, C, int(q_type), bs, _ptr(importance), _ptr(q), _ptr(d), _ptr(ls),
                                     _ptr(step), _ptr(istep), _ptr(ws), ws.numel(), _stream(W)), "gq_gptq_quantize_iq4")
    return q, d, ls, step


def pack_iq4(q_type: int, qweight: torch.Tensor, d: torch.Tensor, ls: Optional[torch.Tensor],
             row_src: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The outputs of gptq_quantize_iq4 as block bytes (gq_pack_iq4): uint8 [R, C/256*136] (IQ4_XS) or [R, C/32*18] (IQ4_NL).
    row_src (int32 [R] on the device): out[r] = the blocks of row row_src[r]; every index must lie in [0, R).  out: None, or
    a contiguous, 16-byte aligned uint8 tensor of exactly the result's bytes on qweight's device (a slot of a stacked buffer),
    written in place and returned as the [R, row bytes] view."""
    _need_cuda(qweight, d, ls, row_src, out)
    xs = _iq4_type("pack_iq4", q_type)
    bs, ts = GGML_QUANT_SIZES[int(q_type)]
    if qweight.dtype != torch.uint8 or qweight.dim() != 2 or qweight.shape[1] % bs or qweight.shape[1] < bs:
        raise _cabi.GQError(f"pack_iq4: qweight must be uint8 [R, C] with C % {bs} == 0; got {qweight.dtype} {tuple(qweight.shape)}")
    R, C = qweight.shape
    if d.dtype != torch.float16 or tuple(d.shape) != (R, C // bs):
        raise _cabi.GQError(f"pack_iq4: d must be fp16 [{R}, {C // bs}]; got {d.dtype} {tuple(d.shape)}")
    if xs and (ls is None or ls.dtype != torch.uint8 or tuple(ls.shape) != (R, C // 32)):
        raise _cabi.GQError(f"pack_iq4: ls must be uint8 [{R}, {C // 32}] for IQ4_XS")
    if row_src is not None:
        if row_src.dtype != torch.int32 or row_src.numel() != R or row_src.device != qweight.device:
            raise _cabi.GQError(f"pack_iq4: row_src must be an int32 [{R}] tensor on {qweight.device}")
        row_src = row_src.contiguous()
    qweight, d = qweight.contiguous(), d.contiguous()
    ls = ls.contiguous() if xs else None
    if out is None:
        out = torch.empty(R, C // bs * ts, dtype=torch.uint8, device=qweight.device)
    else:
        if out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != R * (C // bs * ts) \
                or out.device != qweight.device or out.data_ptr() % 16:
            raise _cabi.GQError(f"pack_iq4: out must be a contiguous, 16-byte aligned uint8 tensor of {R * (C // bs * ts)} bytes "
                                f"on {qweight.device}; got {out.dtype} {tuple(out.shape)}")
        out = out.view(R, C // bs * ts)
    check(lib().gq_pack_iq4(int(q_type), R, C, _ptr(qweight), _ptr(d), _ptr(ls), _ptr(row_src), _ptr(out), _stream(qweight)),
          "gq_pack_iq4")
    return out


def trailing_update(Cm: torch.Tensor, A: torch.Tensor, B: torch.Tensor):
    """Cm -= A @ B (fp32; k-ordered fma chain then one subtraction per element)."""
    _need_cuda(Cm, A, B)
    M, K = A.shape
    K2, N = B.shape
    assert K == K2 and Cm.shape == (M, N) and Cm.stride(1) == 1 and A.stride(1) == 1 and B.stride(1) == 1
    check(lib().gq_trailing_update(_ptr(Cm), Cm.stride(0), _ptr(A), A.stride(0), _ptr(B), B.stride(0), M, N, K,
                                   _stream(Cm)), "gq_trailing_update")
    return Cm


def chol_gemm(Cm: torch.Tensor, A: torch.Tensor, B: torch.Tensor, trans_b: bool, mode: int, k_range: int = 0,
              lower: bool = False, planes: int = 3):
    """One product of the blocked Cholesky chain through the pre-split image kernels (gq_chol_gemm):
    mode 0: Cm -= A op(B), 1: Cm = A op(B), 2: Cm = -(A op(B)); fp32-GEMM accuracy (tolerance class)."""
    _need_cuda(Cm, A, B)
    M, K = A.shape
    N = B.shape[0] if trans_b else B.shape[1]
    assert (B.shape[1] if trans_b else B.shape[0]) == K and Cm.shape == (M, N)
    assert Cm.stride(1) == 1 and A.stride(1) == 1 and B.stride(1) == 1
    ws = _ws(workspace_bytes(_cabi.WS_CHOL_GEMM, M, N, K), Cm.device)
    check(lib().gq_chol_gemm(_ptr(Cm), Cm.stride(0), _ptr(A), A.stride(0), _ptr(B), B.stride(0), M, N, K, int(trans_b),
                             int(mode), int(k_range), int(lower), int(planes), _ptr(ws), ws.numel(), _stream(Cm)),
          "gq_chol_gemm")
    return Cm


def stage_to_host(dst: torch.Tensor, src: torch.Tensor, stream: "torch.cuda.Stream") -> None:
    """src (device, contiguous) -> dst (pinned host memory, same byte size) by a copy kernel on `stream`
    (gq_stage_to_host: no hipMemcpy, no copy-engine lock shared with the launching thread)."""
    _need_cuda(src)
    assert src.is_contiguous() and dst.is_contiguous() and not dst.is_cuda
    n = src.numel() * src.element_size()
    assert dst.numel() * dst.element_size() == n
    check(lib().gq_stage_to_host(_ptr(dst), _ptr(src), n, ctypes.c_void_p(stream.cuda_stream)), "gq_stage_to_host")


def fwd_rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    """LlamaRMSNorm.forward in one pass (gq_fwd_rmsnorm); x [..., C] fp16 / bf16 contiguous, weight [C] of the same dtype."""
    _need_cuda(x, weight)
    assert x.is_contiguous() and weight.is_contiguous() and weight.dtype == x.dtype and weight.numel() == x.shape[-1]
    out = torch.empty_like(x)
    C = x.shape[-1]
    check(lib().gq_fwd_rmsnorm(_ptr(x), _ptr(weight), _ptr(out), x.numel() // C, C, float(eps), _DT[x.dtype], _stream(x)),
          "gq_fwd_rmsnorm")
    return out


def fwd_rmsnorm_ordered(x: torch.Tensor, weight: torch.Tensor, eps: float, want_stats: bool = False):
    """fwd_rmsnorm with the statistics summed in ATen's order (gq_fwd_rmsnorm_ordered; C % 512 == 0).  want_stats: also
    return fp32 [rows, 2] = (mean(x^2), rsqrt(mean + eps)) as the kernel computed them."""
    _need_cuda(x, weight)
    assert x.is_contiguous() and weight.is_contiguous() and weight.dtype == x.dtype and weight.numel() == x.shape[-1]
    out = torch.empty_like(x)
    C = x.shape[-1]
    stats = torch.empty(x.numel() // C, 2, dtype=torch.float32, device=x.device) if want_stats else None
    check(lib().gq_fwd_rmsnorm_ordered(_ptr(x), _ptr(weight), _ptr(out), x.numel() // C, C, float(eps), _DT[x.dtype],
                                       _ptr(stats), _stream(x)), "gq_fwd_rmsnorm_ordered")
    return (out, stats) if want_stats else out


def fwd_rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """apply_rotary_pos_emb on one projection (gq_fwd_rope): x [B, L, H, D] contiguous (q_proj(h).view(B, L, H, D)),
    cos / sin [B, L, D] contiguous, same dtype.  Returns [B, L, H, D]."""
    _need_cuda(x, cos, sin)
    B, L, H, D = x.shape
    assert x.is_contiguous() and cos.is_contiguous() and sin.is_contiguous() and cos.dtype == x.dtype == sin.dtype
    assert cos.shape == (B, L, D) and sin.shape == (B, L, D)
    out = torch.empty_like(x)
    check(lib().gq_fwd_rope(_ptr(x), _ptr(cos), _ptr(sin), _ptr(out), B * L, H, D, _DT[x.dtype], _stream(x)), "gq_fwd_rope")
    return out


def fwd_qk_norm_rope(q: torch.Tensor, k: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                     eps: float, want_stats: bool = False, out=None):
    """Qwen3's q_norm / k_norm (RMSNorm over head_dim) and apply_rotary_pos_emb on both projections in one launch
    (gq_fwd_qk_norm_rope, include/gptq_gguf_qknorm.h): q [B, L, Hq, D], k [B, L, Hk, D] contiguous, wq / wk [D],
    cos / sin [B, L, D] contiguous, one 16-bit dtype, D in 64 / 128 / 256.  Returns (q', k') in the layouts of q and k --
    written into `out` = (q_out, k_out) if given --, and with want_stats also fp32 [B L (Hq + Hk), 2] = (mean(x^2),
    rsqrt(mean + eps)) per row as the kernel computed them, the q rows first."""
    _need_cuda(q, k, wq, wk, cos, sin)
    B, L, Hq, D = q.shape
    Hk = k.shape[2]
    assert k.shape == (B, L, Hk, D) and cos.shape == (B, L, D) and sin.shape == (B, L, D) and wq.shape == (D,) and wk.shape == (D,)
    assert all(t.is_contiguous() and t.dtype == q.dtype for t in (q, k, wq, wk, cos, sin))
    q_out, k_out = out if out is not None else (torch.empty_like(q), torch.empty_like(k))
    assert q_out.shape == q.shape and k_out.shape == k.shape and q_out.is_contiguous() and k_out.is_contiguous()
    assert q_out.dtype == q.dtype == k_out.dtype
    stats = torch.empty(B * L * (Hq + Hk), 2, dtype=torch.float32, device=q.device) if want_stats else None
    check(lib().gq_fwd_qk_norm_rope(_ptr(q), _ptr(k), _ptr(wq), _ptr(wk), _ptr(cos), _ptr(sin), _ptr(q_out), _ptr(k_out), B * L,
                                    Hq, Hk, D, float(eps), _DT[q.dtype], _ptr(stats), _stream(q)), "gq_fwd_qk_norm_rope")
    return (q_out, k_out, stats) if want_stats else (q_out, k_out)


def fwd_silu_mul(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """silu(gate) * up (gq_fwd_silu_mul), fp16 / bf16 contiguous tensors of one shape."""
    _need_cuda(gate, up)
    assert gate.is_contiguous() and up.is_contiguous() and gate.shape == up.shape and gate.dtype == up.dtype
    out = torch.empty_like(gate)
    check(lib().gq_fwd_silu_mul(_ptr(gate), _ptr(up), _ptr(out), gate.numel(), _DT[gate.dtype], _stream(gate)),
          "gq_fwd_silu_mul")
    return out


def group_search(x: torch.Tensor, q_type: int, rmin=-1.0, rdelta=0.1, nstep=20, **mq):
    """make_k_quants / make_quants on a [rows,256] panel (fp32, or fp16/bf16 with per-op rounding).
    Returns (group_scale f32[rows,ng], group_zero f32[rows,ng], d, s, dmin, m)."""
    _need_cuda(x)
    assert x.dim() == 2 and x.shape[1] == 256 and x.stride(1) == 1 and x.dtype in _DT
    rows = x.shape[0]
    ng = 256 // type_info(q_type)["group"]
    dev = x.device
    gs = torch.empty(rows, ng, dtype=torch.float32, device=dev)
    gz = torch.empty(rows, ng, dtype=torch.float32, device=dev)
    d = torch.empty(rows, dtype=torch.float16, device=dev)
    dmin = torch.empty(rows, dtype=torch.float16, device=dev)
    s = torch.empty(rows, ng, dtype=torch.uint8, device=dev)
    m = torch.empty(rows, ng, dtype=torch.uint8, device=dev)
    check(lib().gq_group_search(_ptr(x), _DT[x.dtype], rows, x.stride(0), int(q_type), _search(rmin, rdelta, nstep, **mq),
                                _ptr(gs), _ptr(gz), _ptr(d), _ptr(s), _ptr(dmin), _ptr(m), _stream(x)),
          "gq_group_search")
    t = _idt(q_type)
    return gs, gz, d, s.view(t), dmin, m.view(t)


# ---- scoring (gq_eval_*): logits [..., V] -> one fp32 value per row ----
def _collapse(t: torch.Tensor):
    """(rows, ld) when the leading dimensions of t [..., V] are one run of rows with a single stride, else None."""
    dims = [(n, s) for n, s in zip(t.shape[:-1], t.stride()[:-1]) if n != 1]
    for (_, s0), (n1, s1) in zip(dims, dims[1:]):
        if s0 != n1 * s1:
            return None
    rows = 1
    for n, _ in dims:
        rows *= n
    return rows, (dims[-1][1] if dims else t.shape[-1])


def _row_blocks(*ts):
    """The tensors [..., V] of one leading shape, cut into the fewest pieces each of which is [rows, V] with one row
    stride in every tensor; pieces come in row-major order of the leading shape."""
    cs = [_collapse(t) for t in ts]
    if all(c is not None for c in cs):
        yield cs[0][0], [(t, c[1]) for t, c in zip(ts, cs)]
        return
    for subs in zip(*(t.unbind(0) for t in ts)):
        yield from _row_blocks(*subs)


def _logits_ok(*ts):
    _need_cuda(*ts)
    for t in ts:
        if t.dtype not in _DT or t.dim() < 1 or t.stride(-1) != 1 or t.shape[-1] == 0:
            raise _cabi.GQError(f"eval ops take fp32 / fp16 / bf16 tensors [..., V] with a unit stride over V; got "
                                f"{t.dtype} {tuple(t.shape)} strides {t.stride()}")


def eval_nll(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100, want_lse: bool = False):
    """F.cross_entropy(logits, labels, reduction="none") in one read of the logits (gq_eval_nll): fp32, shape of labels;
    0 where labels == ignore_index.  want_lse: also the rows' logsumexp.  Row strides are passed on, nothing is copied.
    A label outside [0, V) raises GQError (this op waits for the stream to find out)."""
    _logits_ok(logits)
    _need_cuda(labels)
    lead, V = logits.shape[:-1], logits.shape[-1]
    if tuple(labels.shape) != tuple(lead) or labels.dtype != torch.int64:
        raise _cabi.GQError(f"eval_nll: labels must be int64 of shape {tuple(lead)}, got {labels.dtype} {tuple(labels.shape)}")
    lab = labels.contiguous().view(-1)
    nll = torch.empty(lab.numel(), dtype=torch.float32, device=logits.device)
    lse = torch.empty_like(nll) if want_lse else None
    a = 0
    for rows, ((x, ld),) in _row_blocks(logits):
        if rows:
            check(lib().gq_eval_nll(_ptr(x), _DT[x.dtype], rows, V, ld, _ptr(lab[a:a + rows]), int(ignore_index),
                                    _ptr(nll[a:a + rows]), _ptr(lse[a:a + rows] if want_lse else None), _stream(x)),
                  "gq_eval_nll")
        a += rows
    return (nll.view(lead), lse.view(lead)) if want_lse else nll.view(lead)


def eval_kl(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Per row KL(softmax(target) || softmax(logits)) = F.kl_div(log_softmax(logits), log_softmax(target), log_target=True)
    summed over V, in one read of both (gq_eval_kl): fp32, the leading shape.  Views are read in place."""
    _logits_ok(logits, target)
    if logits.shape != target.shape:
        raise _cabi.GQError(f"eval_kl: logits {tuple(logits.shape)} and target {tuple(target.shape)} differ in shape")
    lead, V = logits.shape[:-1], logits.shape[-1]
    kl = torch.empty(lead, dtype=torch.float32, device=logits.device).view(-1)
    a = 0
    for rows, ((x, ld), (t, ldt)) in _row_blocks(logits, target):
        if rows:
            check(lib().gq_eval_kl(_ptr(x), _DT[x.dtype], _ptr(t), _DT[t.dtype], rows, V, ld, ldt, _ptr(kl[a:a + rows]),
                                   _stream(x)), "gq_eval_kl")
        a += rows
    return kl.view(lead)


def eval_kl_sparse(logits: torch.Tensor, target_vals: torch.Tensor, target_ids: torch.Tensor) -> torch.Tensor:
    """The same KL over K columns per row: logits.gather(-1, target_ids) against target_vals, both softmaxes over the K
    entries (gq_eval_kl_sparse; K <= 4096, ids int64 in [0, V)).  fp32, the leading shape."""
    _logits_ok(logits, target_vals)
    _need_cuda(target_ids)
    lead, V, K = logits.shape[:-1], logits.shape[-1], target_vals.shape[-1]
    if tuple(target_vals.shape[:-1]) != tuple(lead) or target_ids.shape != target_vals.shape or target_ids.dtype != torch.int64:
        raise _cabi.GQError(f"eval_kl_sparse: target_vals / target_ids must be {tuple(lead)} + (K,), ids int64; got "
                            f"{tuple(target_vals.shape)} and {target_ids.dtype} {tuple(target_ids.shape)}")
    tv, ti = target_vals.contiguous().view(-1, K), target_ids.contiguous().view(-1, K)
    kl = torch.empty(tv.shape[0], dtype=torch.float32, device=logits.device)
    a = 0
    for rows, ((x, ld),) in _row_blocks(logits):
        if rows:
            check(lib().gq_eval_kl_sparse(_ptr(x), _DT[x.dtype], rows, V, ld, _ptr(tv[a:a + rows]), _DT[tv.dtype],
                                          _ptr(ti[a:a + rows]), K, _ptr(kl[a:a + rows]), _stream(x)), "gq_eval_kl_sparse")
        a += rows
    return kl.view(lead)


# ---- layer error estimate (gq_quad_form): sum_r d_r H~ d_r^T, d = A - B ----
def _qf_rows(t: torch.Tensor) -> torch.Tensor:
    """t [R, C] as the kernel can read it: unit column stride and 16-byte aligned rows; a copy only when that fails."""
    es = t.element_size()
    if t.stride(1) == 1 and t.data_ptr() % 16 == 0 and (t.shape[0] == 1 or (t.stride(0) >= t.shape[1] and t.stride(0) * es % 16 == 0)):
        return t
    return t.contiguous()


def quad_form(A: torch.Tensor, H: torch.Tensor, B: Optional[torch.Tensor] = None,
              ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """((D @ H~) * D).sum() with D = A - B (D = A when B is None), as a 0-dim fp64 device tensor (gq_quad_form): the two
    sums of evopress/src/error_estimator.py:101-102.  A, B [R, C] fp32 / fp16 / bf16, read in their own dtype and with
    their own row stride (a view is copied only when its rows are not 16-byte aligned); H [C, C] fp32 symmetric, a zero
    on its diagonal counts as 1 and H is not written.  No host read."""
    _need_cuda(A, H, B, ws)
    if A.dim() != 2 or A.dtype not in _DT or (B is not None and (B.shape != A.shape or B.dtype not in _DT)):
        raise _cabi.GQError(f"quad_form: A and B must be [R, C] fp32 / fp16 / bf16 tensors of one shape; got "
                            f"{A.dtype} {tuple(A.shape)} and {None if B is None else (B.dtype, tuple(B.shape))}")
    R, C = A.shape
    for t in (H, B, ws):
        if t is not None and t.device != A.device:
            raise _cabi.GQError(f"quad_form: every tensor must be on A's device {A.device}; got one on {t.device}")
    if ws is not None and (not ws.is_contiguous() or ws.data_ptr() % 8):
        raise _cabi.GQError("quad_form: ws must be contiguous and 8-byte aligned")
    if H.dtype != torch.float32 or tuple(H.shape) != (C, C) or not H.is_contiguous():
        raise _cabi.GQError(f"quad_form: H must be a contiguous fp32 [{C}, {C}] tensor; got {H.dtype} {tuple(H.shape)}")
    A = _qf_rows(A)
    B = _qf_rows(B) if B is not None else None
    need = int(lib().gq_quad_form_workspace_bytes(R, C))
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = _ws(need, A.device)
    out = torch.empty((), dtype=torch.float64, device=A.device)
    lda = A.stride(0) if R > 1 else max(A.stride(0), C)
    ldb = 0 if B is None else (B.stride(0) if R > 1 else max(B.stride(0), C))
    check(lib().gq_quad_form(_ptr(A), _DT[A.dtype], lda, _ptr(B), _DT[B.dtype] if B is not None else 0, ldb, _ptr(H), R, C,
                             _ptr(out), _ptr(ws), ws.numel() * ws.element_size(), _stream(A)), "gq_quad_form")
    return out


# ---- layer error estimate of a stacked expert tensor (gq_quad_form_experts): quad_form per expert, two launches ----
QUAD_EXPERTS_MAX = _cabi.QUAD_EXPERTS_MAX


def _qf_experts(t: torch.Tensor) -> torch.Tensor:
    """t [E, R, C] as the kernel can read it: every t[e] as _qf_rows wants it, the expert stride a multiple of 16 bytes and
    no smaller than a matrix; a copy only when that fails (the halves of a fused gate_up_proj are read in place)."""
    E, R, C = t.shape
    es = t.element_size()
    ld = t.stride(1) if R > 1 else max(t.stride(1), C)
    rows = t.stride(2) == 1 and t.data_ptr() % 16 == 0 and (R == 1 or (t.stride(1) >= C and t.stride(1) * es % 16 == 0))
    if rows and (E == 1 or (t.stride(0) >= (R - 1) * ld + C and t.stride(0) * es % 16 == 0)):
        return t
    return t.contiguous()


def quad_form_experts(A: torch.Tensor, H: torch.Tensor, B: Optional[torch.Tensor] = None,
                      ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[e] = quad_form(A[e], H[e], B[e]) for the E experts of a stacked tensor, bit for bit, as an fp64 [E] device tensor
    in two launches whatever E (gq_quad_form_experts).  A, B [E, R, C] fp32 / fp16 / bf16 views, each in its own dtype and
    with its own strides (`gate_up_proj[:, :I]` and `gate_up_proj[:, I:]` are read in place; a view is copied only when its
    rows or its expert stride are not 16-byte aligned); H [E, C, C] fp32 contiguous, every H[e] symmetric, a zero on a
    diagonal counts as 1 (an all-zero H[e] is the identity) and H is not written.  No host read."""
    _need_cuda(A, H, B, ws)
    if A.dim() != 3 or A.dtype not in _DT or 0 in A.shape or (B is not None and (B.shape != A.shape or B.dtype not in _DT)):
        raise _cabi.GQError(f"quad_form_experts: A and B must be [E, R, C] fp32 / fp16 / bf16 tensors of one shape; got "
                            f"{A.dtype} {tuple(A.shape)} and {None if B is None else (B.dtype, tuple(B.shape))}")
    E, R, C = A.shape
    for t in (H, B, ws):
        if t is not None and t.device != A.device:
            raise _cabi.GQError(f"quad_form_experts: every tensor must be on A's device {A.device}; got one on {t.device}")
    if ws is not None and (not ws.is_contiguous() or ws.data_ptr() % 8):
        raise _cabi.GQError("quad_form_experts: ws must be contiguous and 8-byte aligned")
    if H.dtype != torch.float32 or tuple(H.shape) != (E, C, C) or not H.is_contiguous():
        raise _cabi.GQError(f"quad_form_experts: H must be a contiguous fp32 [{E}, {C}, {C}] tensor; got {H.dtype} "
                            f"{tuple(H.shape)}")
    A = _qf_experts(A)
    B = _qf_experts(B) if B is not None else None
    need = int(lib().gq_quad_form_experts_workspace_bytes(E, R, C))
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = _ws(need, A.device)
    out = torch.empty(E, dtype=torch.float64, device=A.device)

    def geom(t):  # (ld, expert stride); torch reports any stride for an extent of 1
        ld = t.stride(1) if R > 1 else max(t.stride(1), C)
        return ld, (t.stride(0) if E > 1 else R * ld)

    (lda, sa), (ldb, sb) = geom(A), (geom(B) if B is not None else (0, 0))
    check(lib().gq_quad_form_experts(_ptr(A), _DT[A.dtype], lda, sa, _ptr(B), _DT[B.dtype] if B is not None else 0, ldb, sb,
                                     _ptr(H), E, R, C, _ptr(out), _ptr(ws), ws.numel() * ws.element_size(), _stream(A)),
          "gq_quad_form_experts")
    return out


# ---- level switch of the bit-width search (gq_level_switch): stored levels -> live weights, one call ----
def level_switch(jobs) -> None:
    """Apply a list of jobs (src, dst, kind, row_src) in ONE gq_level_switch call on the current stream of their device.
    dst: contiguous [R, C] fp32 / fp16 / bf16, written in place.  kind a K-quant q_type (10..14), Q8_0 (8), IQ4_NL (20) or IQ4_XS (23): src uint8, R rows
    of C / 256 packed blocks (Q8_0: C / 32 blocks of 34 bytes; any 1-D / 2-D contiguous view of exactly those bytes); kind None: src a dense
    contiguous [R, C] tensor, cast as .to(dst.dtype).  row_src: None or int32 [R], dst[r] = f(src[row_src[r]]); every index
    must lie in [0, R) -- the kernel does not check.  Returns None; no host read, no allocation on the device."""
    jobs = list(jobs)
    if not jobs:
        return None
    dev = jobs[0][1].device
    table = (_cabi.SwitchJob * len(jobs))()
    for i, (src, dst, kind, row_src) in enumerate(jobs):
        _need_cuda(src, dst, row_src)
        for t in (src, dst, row_src):
            if t is not None and t.device != dev:
                raise _cabi.GQError(f"level_switch: job {i}: every tensor must be on one device ({dev}); got one on {t.device}")
        if dst.dim() != 2 or not dst.is_contiguous() or dst.dtype not in _DT:
            raise _cabi.GQError(f"level_switch: job {i}: dst must be a contiguous [R, C] fp32 / fp16 / bf16 tensor; got "
                                f"{dst.dtype} {tuple(dst.shape)} strides {tuple(dst.stride())}")
        R, C = dst.shape
        if not src.is_contiguous():
            raise _cabi.GQError(f"level_switch: job {i}: src must be contiguous")
        if kind is None:
            if src.dtype not in _DT or tuple(src.shape) != (R, C):
                raise _cabi.GQError(f"level_switch: job {i}: a dense src must be fp32 / fp16 / bf16 {(R, C)}; got {src.dtype} "
                                    f"{tuple(src.shape)}")
            k = _DT[src.dtype]
        else:
            k = int(kind)
            bs, ts = block_geometry(k)
            need = R * (C // bs) * ts
            if src.dtype != torch.uint8 or C % bs or src.numel() != need:
                raise _cabi.GQError(f"level_switch: job {i}: packed src of q_type {k} for {(R, C)} must be {need} uint8; got "
                                    f"{src.dtype} {tuple(src.shape)}")
        if row_src is not None and (row_src.dtype != torch.int32 or row_src.numel() != R or not row_src.is_contiguous()):
            raise _cabi.GQError(f"level_switch: job {i}: row_src must be a contiguous int32 [{R}] tensor")
        table[i] = _cabi.SwitchJob(src.data_ptr(), dst.data_ptr(), row_src.data_ptr() if row_src is not None else None,
                                   R, C, k, _DT[dst.dtype])
    check(lib().gq_level_switch(table, len(jobs), _stream(jobs[0][1])), "gq_level_switch")
    return None


# ---- level switch of stacked expert tensors (gq_level_switch_experts): one job per [E, R, C] tensor, one call ----
SWITCH_EXPERTS_MAX_JOBS = _cabi.SWITCH_EXPERTS_MAX_JOBS


def level_switch_experts(jobs) -> None:
    """Apply a list of jobs (src, dst_view, kind) in ONE gq_level_switch_experts call on the current stream of their device.
    dst_view: an [E, R, C] fp32 / fp16 / bf16 view whose last two dimensions are contiguous, written in place; its stride(0) is
    the expert stride, so `gate_up_proj[:, :I]`, `gate_up_proj[:, I:]` and `down_proj` of a fused experts module are all
    destinations (nothing outside the view is written).  kind a K-quant q_type (10..14), Q8_0 (8), IQ4_NL (20) or IQ4_XS (23):
    src uint8, E * R rows of packed blocks as in the file (any contiguous view of exactly those bytes); kind None: src a dense
    contiguous [E, R, C] tensor, cast as .to(dst.dtype).  The values are those of level_switch with the E per-expert jobs.
    Returns None; no host read, no allocation on the device."""
    jobs = list(jobs)
    if not jobs:
        return None
    dev = jobs[0][1].device
    table = (_cabi.SwitchExpertsJob * len(jobs))()
    for i, (src, dst, kind) in enumerate(jobs):
        _need_cuda(src, dst)
        for t in (src, dst):
            if t.device != dev:
                raise _cabi.GQError(f"level_switch_experts: job {i}: every tensor must be on one device ({dev}); got one on "
                                    f"{t.device}")
        if dst.dim() != 3 or dst.dtype not in _DT or 0 in dst.shape or not dst[0].is_contiguous():
            raise _cabi.GQError(f"level_switch_experts: job {i}: dst must be an [E, R, C] fp32 / fp16 / bf16 view with contiguous "
                                f"[R, C] matrices; got {dst.dtype} {tuple(dst.shape)} strides {tuple(dst.stride())}")
        E, R, C = dst.shape
        stride = dst.stride(0) if E > 1 else R * C  # (torch reports any stride for an extent of 1)
        if not src.is_contiguous():
            raise _cabi.GQError(f"level_switch_experts: job {i}: src must be contiguous")
        if kind is None:
            if src.dtype not in _DT or tuple(src.shape) != (E, R, C):
                raise _cabi.GQError(f"level_switch_experts: job {i}: a dense src must be fp32 / fp16 / bf16 {(E, R, C)}; got "
                                    f"{src.dtype} {tuple(src.shape)}")
            k = _DT[src.dtype]
        else:
            k = int(kind)
            bs, ts = block_geometry(k)
            need = E * R * (C // bs) * ts
            if src.dtype != torch.uint8 or C % bs or src.numel() != need:
                raise _cabi.GQError(f"level_switch_experts: job {i}: packed src of q_type {k} for {(E, R, C)} must be {need} uint8; "
                                    f"got {src.dtype} {tuple(src.shape)}")
        table[i] = _cabi.SwitchExpertsJob(src.data_ptr(), dst.data_ptr(), E, R, C, stride, k, _DT[dst.dtype])
    check(lib().gq_level_switch_experts(table, len(jobs), _stream(jobs[0][1])), "gq_level_switch_experts")
    return None


# ---- the packed-weight forward (gq_linear_packed, gq_gemv_packed): y = x W^T with W given as GGUF block bytes ----
GEMV_MAX_T = _cabi.GEMV_MAX_T


def _packed_args(who: str, q_type, blocks, x, row_src):
    """The argument checks the two packed forwards share -> (k, R, C, T)."""
    _need_cuda(blocks, x, row_src)
    k = int(q_type)
    bs, ts = block_geometry(k)
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise _cabi.GQError(f"{who}: x must be fp16 or bf16 (there is no fp32 path); got {x.dtype}")
    if x.dim() < 1 or not x.is_contiguous() or x.numel() == 0:
        raise _cabi.GQError(f"{who}: x must be a non-empty contiguous [..., C] tensor; got {tuple(x.shape)} strides "
                            f"{tuple(x.stride())}")
    for t in (blocks, row_src):
        if t is not None and t.device != x.device:
            raise _cabi.GQError(f"{who}: every tensor must be on one device ({x.device}); got one on {t.device}")
    C = x.shape[-1]
    if C % 256:
        raise _cabi.GQError(f"{who}: C={C} (C % 256 != 0; Q8_0 and IQ4_NL included)")
    row_bytes = C // bs * ts
    if (blocks.dtype != torch.uint8 or blocks.dim() not in (1, 2) or not blocks.is_contiguous() or blocks.numel() == 0
            or blocks.numel() % row_bytes or (blocks.dim() == 2 and blocks.shape[1] != row_bytes)):
        raise _cabi.GQError(f"{who}: packed blocks of q_type {k} for C={C} must be contiguous uint8, R rows of "
                            f"{row_bytes} bytes; got {blocks.dtype} {tuple(blocks.shape)}")
    R, T = blocks.numel() // row_bytes, x.numel() // C
    if row_src is not None and (row_src.dtype != torch.int32 or row_src.numel() != R or not row_src.is_contiguous()):
        raise _cabi.GQError(f"{who}: row_src must be a contiguous int32 [{R}] tensor")
    return k, R, C, T


def linear_packed(q_type: int, blocks: torch.Tensor, x: torch.Tensor, row_src: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [..., C] fp16 / bf16, contiguous, times the weight [R, C] that `blocks` holds packed (a K-quant q_type 10..14 or
    Q8_0 8, IQ4_NL 20 or IQ4_XS 23; uint8, any 1-D / 2-D contiguous view of exactly R rows of block_geometry's blocks)
    -> y [..., R] in x's dtype, on the current stream of x's device.  C % 256 == 0 for every type.  The weight operand is
    bit for bit dequantize_blocks(q_type, blocks, x.dtype, row_src); fp32 accumulation, one rounding.  row_src: None or
    int32 [R], row r of the weight is packed row row_src[r]; every index must lie in [0, R) -- the kernel does not check.
    No dense weight, no workspace, no host read."""
    k, R, C, T = _packed_args("linear_packed", q_type, blocks, x, row_src)
    y = torch.empty(*x.shape[:-1], R, dtype=x.dtype, device=x.device)
    check(lib().gq_linear_packed(k, _ptr(blocks), _ptr(row_src), R, C, _ptr(x), T, _DT[x.dtype], _ptr(y), _stream(x)),
          "gq_linear_packed")
    return y


def gemv_packed(q_type: int, blocks: torch.Tensor, x: torch.Tensor, row_src: Optional[torch.Tensor] = None) -> torch.Tensor:
    """linear_packed for the few tokens of a decode step (gq_gemv_packed): the same arguments, the same weight operand bits,
    fp32 accumulation and one rounding, for 1 <= T = x.numel() // C <= GEMV_MAX_T tokens; the two differ by fp32 summation
    order only.  One stream over the weight bytes that fills the device at T = 1, where linear_packed's token tile is empty."""
    k, R, C, T = _packed_args("gemv_packed", q_type, blocks, x, row_src)
    if T > GEMV_MAX_T:
        raise _cabi.GQError(f"gemv_packed: T={T} tokens, at most GEMV_MAX_T={GEMV_MAX_T} (linear_packed takes more tokens)")
    y = torch.empty(*x.shape[:-1], R, dtype=x.dtype, device=x.device)
    check(lib().gq_gemv_packed(k, _ptr(blocks), _ptr(row_src), R, C, _ptr(x), T, _DT[x.dtype], _ptr(y), _stream(x)),
          "gq_gemv_packed")
    return y


# ---- the grouped expert GEMV of a packed MoE layer's decode step (gq_gemv_packed_experts) ----
MOE_MAX_PAIRS = _cabi.MOE_MAX_PAIRS


def _packed_experts_args(who: str, q_type, blocks, E, R, x, idx, idx_check, pairs_per_row, max_E, max_E_name, max_P, max_P_name,
                         E_first: bool):
    """The argument checks the two grouped expert ops share -> (k, E, R, C, x_rows, P, ppr).  idx: the op's index tensors;
    idx_check() refuses them in the op's own words and returns P.  E_first: the op names a bad E / R before its index tensors
    (linear_packed_experts), else after the pairs (gemv_packed_experts).  _need_cuda comes last: the refusals before it name
    their value for tensors on any device."""
    k, E, R, ppr = int(q_type), int(E), int(R), int(pairs_per_row)
    bs, ts = block_geometry(k)
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise _cabi.GQError(f"{who}: x must be fp16 or bf16 (there is no fp32 path); got {x.dtype}")
    if x.dim() != 2 or not x.is_contiguous() or x.numel() == 0:
        raise _cabi.GQError(f"{who}: x must be a non-empty contiguous [x_rows, C] tensor; got {tuple(x.shape)} strides "
                            f"{tuple(x.stride())}")
    for t in (blocks, *idx):
        if t.device != x.device:
            raise _cabi.GQError(f"{who}: every tensor must be on one device ({x.device}); got one on {t.device}")
    x_rows, C = x.shape
    if C % 256:
        raise _cabi.GQError(f"{who}: C={C} (C % 256 != 0; Q8_0 and IQ4_NL included)")

    def check_E():
        if E < 1 or E > max_E or R < 1:
            raise _cabi.GQError(f"{who}: E={E}, R={R} (1 <= E <= {max_E_name}, R >= 1)")

    if E_first:
        check_E()
    P = idx_check()
    if P < 1 or P > max_P:
        raise _cabi.GQError(f"{who}: P={P} pairs (not in [1, {max_P_name}={max_P}])")
    if ppr < 1 or x_rows * ppr != P:
        raise _cabi.GQError(f"{who}: x_rows={x_rows} * pairs_per_row={ppr} != P={P}")
    if not E_first:
        check_E()
    need = E * R * (C // bs) * ts
    if blocks.dtype != torch.uint8 or not blocks.is_contiguous() or blocks.numel() != need:
        raise _cabi.GQError(f"{who}: packed blocks of q_type {k} for [E={E}, R={R}, C={C}] must be {need} contiguous uint8; "
                            f"got {blocks.dtype} {tuple(blocks.shape)}")
    _need_cuda(blocks, x, *idx)
    return k, E, R, C, x_rows, P, ppr


def gemv_packed_experts(q_type: int, blocks: torch.Tensor, E: int, R: int, x: torch.Tensor, pair_expert: torch.Tensor,
                        pairs_per_row: int) -> torch.Tensor:
    """y [P, R] with y[p] = W[pair_expert[p]] x[p // pairs_per_row] in ONE launch: `blocks` holds the stacked expert tensor
    [E, R, C] packed (a K-quant q_type 10..14, Q8_0 8, IQ4_NL 20 or IQ4_XS 23; contiguous uint8 of exactly E * R rows of blocks, any
    shape), x is contiguous [x_rows, C] fp16 / bf16, pair_expert int32 [P] on the device with P = x_rows * pairs_per_row,
    1 <= P <= MOE_MAX_PAIRS.  pairs_per_row = K: gate / up (x the hidden states, the pairs in the row-major order of the
    router's [T, K] index); pairs_per_row = 1: down (x the [P, I] activation).  Row p is bit for bit
    gemv_packed(q_type, expert pair_expert[p]'s slice, x[p // pairs_per_row]).  An id outside [0, E) is not checked: that
    pair is skipped and its row of y stays as torch.empty left it.  The ids are never read by the host: no synchronisation."""
    def pairs():
        if pair_expert.dtype != torch.int32 or pair_expert.dim() != 1 or not pair_expert.is_contiguous():
            raise _cabi.GQError(f"gemv_packed_experts: pair_expert must be a contiguous int32 [P] tensor; got {pair_expert.dtype} "
                                f"{tuple(pair_expert.shape)}")
        return pair_expert.numel()

    k, E, R, C, x_rows, P, ppr = _packed_experts_args("gemv_packed_experts", q_type, blocks, E, R, x, (pair_expert,), pairs,
                                                      pairs_per_row, 65535, "65535", MOE_MAX_PAIRS, "MOE_MAX_PAIRS", E_first=False)
    y = torch.empty(P, R, dtype=x.dtype, device=x.device)
    check(lib().gq_gemv_packed_experts(k, _ptr(blocks), E, R, C, _ptr(x), x_rows, _ptr(pair_expert), P, ppr, _DT[x.dtype],
                                       _ptr(y), _stream(x)), "gq_gemv_packed_experts")
    return y


# ---- the packed MoE prefill: device-side routing (gq_moe_route) and the grouped expert GEMM (gq_linear_packed_experts) ----
MOE_ROUTE_MAX_EXPERTS = _cabi.MOE_ROUTE_MAX_EXPERTS
MOE_ROUTE_MAX_PAIRS = _cabi.MOE_ROUTE_MAX_PAIRS


def moe_route(pair_expert: torch.Tensor, E: int):
    """The router's pairs sorted by expert, on the device, in one launch: pair_expert int32 [P] (the [T, K] index in row-major
    order), 1 <= P <= MOE_ROUTE_MAX_PAIRS, 1 <= E <= MOE_ROUTE_MAX_EXPERTS -> (expert_start int32 [E + 1], order int32 [P]).
    order[expert_start[e] : expert_start[e + 1]] are the pairs that name expert e, ascending (a stable sort); an id outside
    [0, E) -- E for a masked pair, negative ids -- is in no run, expert_start[E] counts the others and order holds -1 from
    there on.  Both outputs are defined for every input.  The ids are never read by the host: no synchronisation."""
    E = int(E)
    who = "moe_route"
    if pair_expert.dtype != torch.int32 or pair_expert.dim() != 1 or not pair_expert.is_contiguous():
        raise _cabi.GQError(f"{who}: pair_expert must be a contiguous int32 [P] tensor; got {pair_expert.dtype} "
                            f"{tuple(pair_expert.shape)}")
    P = pair_expert.numel()
    if P < 1 or P > MOE_ROUTE_MAX_PAIRS:
        raise _cabi.GQError(f"{who}: P={P} pairs (not in [1, MOE_ROUTE_MAX_PAIRS={MOE_ROUTE_MAX_PAIRS}])")
    if E < 1 or E > MOE_ROUTE_MAX_EXPERTS:
        raise _cabi.GQError(f"{who}: E={E} experts (not in [1, MOE_ROUTE_MAX_EXPERTS={MOE_ROUTE_MAX_EXPERTS}])")
    _need_cuda(pair_expert)
    expert_start = torch.empty(E + 1, dtype=torch.int32, device=pair_expert.device)
    order = torch.empty(P, dtype=torch.int32, device=pair_expert.device)
    check(lib().gq_moe_route(_ptr(pair_expert), P, E, _ptr(expert_start), _ptr(order), _stream(pair_expert)), "gq_moe_route")
    return expert_start, order


def linear_packed_experts(q_type: int, blocks: torch.Tensor, E: int, R: int, x: torch.Tensor, route, pairs_per_row: int) -> torch.Tensor:
    """y [P, R] with y[p] = W[expert of pair p] x[p // pairs_per_row] for every pair of `route` = moe_route(pair_expert, E) in
    ONE launch of the tile GEMM: `blocks` holds the stacked expert tensor [E, R, C] packed (a K-quant q_type 10..14, Q8_0 8, IQ4_NL 20 or IQ4_XS 23;
    contiguous uint8 of exactly E * R rows of C / 256 blocks, any shape), x is contiguous [x_rows, C] fp16 / bf16 with
    x_rows * pairs_per_row = P = route[1].numel().  pairs_per_row = K: gate / up; pairs_per_row = 1: down.  The tokens of an
    expert are gathered and the results scattered to pair order inside the kernel.  Row p is bit for bit
    linear_packed(q_type, that expert's slice, x[p // pairs_per_row]).  A pair that is in no run of the route (a masked
    pair) is skipped and its row of y stays as torch.empty left it.  Nothing is read by the host: no synchronisation."""
    expert_start, order = route

    def pairs():
        for name, t, n in (("expert_start", expert_start, int(E) + 1), ("order", order, order.numel())):
            if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.numel() != n:
                raise _cabi.GQError(f"linear_packed_experts: route: {name} must be a contiguous int32 [{n}] tensor (moe_route's "
                                    f"output for E={int(E)}); got {t.dtype} {tuple(t.shape)}")
        return order.numel()

    k, E, R, C, x_rows, P, ppr = _packed_experts_args(
        "linear_packed_experts", q_type, blocks, E, R, x, route, pairs, pairs_per_row, MOE_ROUTE_MAX_EXPERTS,
        f"MOE_ROUTE_MAX_EXPERTS={MOE_ROUTE_MAX_EXPERTS}", MOE_ROUTE_MAX_PAIRS, "MOE_ROUTE_MAX_PAIRS", E_first=True)
    y = torch.empty(P, R, dtype=x.dtype, device=x.device)
    check(lib().gq_linear_packed_experts(k, _ptr(blocks), E, R, C, _ptr(x), x_rows, ppr, _ptr(expert_start), _ptr(order), P,
                                         _DT[x.dtype], _ptr(y), _stream(x)), "gq_linear_packed_experts")
    return y


# ---- the calibration forward of fused (dense) experts: the combine with transformers' roundings (gq_fwd_moe_combine) ----
MOE_COMBINE_MAX_K = _cabi.MOE_COMBINE_MAX_K


def fwd_moe_combine(y: torch.Tensor, pair_expert: torch.Tensor, route, w: torch.Tensor, E: int) -> torch.Tensor:
    """out [T, H] = what transformers' MixtralExperts.forward leaves in final_hidden_states, in ONE launch: y [P, H] fp16 / bf16
    contiguous holds the down-projection outputs in expert-sorted order (row s belongs to pair route[1][s]), pair_expert int32
    [P] is the router's [T, K] index TRANSPOSED and flattened (pair p = k T + t) and route = moe_route(pair_expert, E); w [T, K]
    contiguous, fp32 or y's dtype, 1 <= K <= MOE_COMBINE_MAX_K, H % 8 == 0.  Per token and element: the products
    round(float(y) float(w)) are added in ascending expert id (ties by k) to an accumulator that starts at +0 and is rounded to
    y's dtype after every add; a pair with an id outside [0, E) contributes nothing (include/gptq_gguf_moe_calib.h).  Nothing
    is read by the host: no synchronisation."""
    who = "fwd_moe_combine"
    expert_start, order = route
    E = int(E)
    if y.dtype not in (torch.float16, torch.bfloat16) or y.dim() != 2 or not y.is_contiguous():
        raise _cabi.GQError(f"{who}: y must be a contiguous fp16 or bf16 [P, H] tensor; got {y.dtype} {tuple(y.shape)}")
    if w.dim() != 2 or not w.is_contiguous() or w.dtype not in (torch.float32, y.dtype):
        raise _cabi.GQError(f"{who}: w must be a contiguous [T, K] tensor, fp32 or {y.dtype}; got {w.dtype} {tuple(w.shape)}")
    T, K = w.shape
    P, H = y.shape
    if K < 1 or K > MOE_COMBINE_MAX_K:
        raise _cabi.GQError(f"{who}: K={K} experts per token (not in [1, MOE_COMBINE_MAX_K={MOE_COMBINE_MAX_K}])")
    if T < 1 or T * K != P or P > MOE_ROUTE_MAX_PAIRS:
        raise _cabi.GQError(f"{who}: T={T} * K={K} != P={P} rows of y (or not in [1, MOE_ROUTE_MAX_PAIRS={MOE_ROUTE_MAX_PAIRS}])")
    if H < 8 or H % 8:
        raise _cabi.GQError(f"{who}: H={H} (H % 8 == 0)")
    if E < 1 or E > MOE_ROUTE_MAX_EXPERTS:
        raise _cabi.GQError(f"{who}: E={E} experts (not in [1, MOE_ROUTE_MAX_EXPERTS={MOE_ROUTE_MAX_EXPERTS}])")
    for name, t, n in (("pair_expert", pair_expert, P), ("expert_start", expert_start, E + 1), ("order", order, P)):
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.numel() != n:
            raise _cabi.GQError(f"{who}: {name} must be a contiguous int32 [{n}] tensor; got {t.dtype} {tuple(t.shape)}")
    _need_cuda(y, pair_expert, expert_start, order, w)
    out = torch.empty(T, H, dtype=y.dtype, device=y.device)
    check(lib().gq_fwd_moe_combine(_ptr(y), _ptr(pair_expert), _ptr(expert_start), _ptr(order), _ptr(w), _DT[w.dtype], T, K, E, H,
                                   _DT[y.dtype], _ptr(out), _stream(y)), "gq_fwd_moe_combine")
    return out


# ---- the vocabulary ends of a packed model: the embedding lookup from block bytes, the sampler on the logits ----
def embed_packed(q_type: int, blocks: torch.Tensor, ids: torch.Tensor, out_dtype=torch.float16) -> torch.Tensor:
    """The rows `ids` of the embedding table that `blocks` holds packed (uint8 [V, C/block*type_size], a K-quant or Q8_0)
    -> [*ids.shape, C] in out_dtype: gq_dequantize_blocks with ids.numel() output rows and the ids as its row gather, so bit
    for bit dequantize_blocks(q_type, blocks, out_dtype)[ids].  ids: int32 or int64 on the blocks' device, every id in
    [0, V) -- the kernel does not check.  An empty ids gives an empty result without a launch."""
    _need_cuda(blocks, ids)
    bs, ts = block_geometry(q_type)
    if blocks.dtype != torch.uint8 or blocks.dim() != 2 or blocks.shape[0] < 1 or blocks.shape[1] < ts or blocks.shape[1] % ts:
        raise _cabi.GQError(f"embed_packed: packed blocks of q_type {int(q_type)} must be uint8 [V, C/{bs}*{ts}]; got "
                            f"{blocks.dtype} {tuple(blocks.shape)}")
    if ids.dtype not in (torch.int32, torch.int64):
        raise _cabi.GQError(f"embed_packed: ids must be int32 or int64, got {ids.dtype}")
    if ids.device != blocks.device:
        raise _cabi.GQError(f"embed_packed: ids on {ids.device}, blocks on {blocks.device}")
    if out_dtype not in _DT:
        raise _cabi.GQError(f"embed_packed: out_dtype must be fp32, fp16 or bf16, got {out_dtype}")
    blocks = blocks.contiguous()
    C, n = blocks.shape[1] // ts * bs, ids.numel()
    out = torch.empty(*ids.shape, C, dtype=out_dtype, device=blocks.device)
    if n:
        rows = ids.reshape(-1).to(torch.int32).contiguous()
        check(lib().gq_dequantize_blocks(int(q_type), _ptr(blocks), n, C, _ptr(rows), _ptr(out), _DT[out_dtype],
                                         _stream(blocks)), "gq_dequantize_blocks")
    return out


SAMPLE_MAX_K = _cabi.SAMPLE_MAX_K


def sample_logits(logits: torch.Tensor, u: Optional[torch.Tensor], top_k: int, top_p: float = 1.0,
                  temperature: float = 1.0) -> torch.Tensor:
    """logits [B, V] fp32 / fp16 / bf16 (unit stride over V, any row stride >= V) -> int64 [B] token ids in one launch
    (gq_sample_logits; include/gptq_gguf_sample.h is the contract): temperature, then the top_k tokens by (logit descending,
    index ascending), then the top_p nucleus, then the inverse CDF at u[b].  u: fp32 [B] in [0, 1) on the device, the
    caller's random numbers; may be None when temperature == 0 (the argmax, lowest index among equals).  A row with a NaN
    or a non-finite maximum gives -1.  1 <= top_k <= SAMPLE_MAX_K: there is no unbounded nucleus, and no value is
    substituted for top_k = 0.  No host synchronise."""
    _need_cuda(logits, u)
    if logits.dtype not in _DT or logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1 or logits.stride(1) != 1:
        raise _cabi.GQError(f"sample_logits: logits must be a non-empty fp32 / fp16 / bf16 [B, V] tensor with a unit stride "
                            f"over V; got {logits.dtype} {tuple(logits.shape)} strides {tuple(logits.stride())}")
    B, V = logits.shape
    ld = logits.stride(0) if B > 1 else V
    if ld < V:
        raise _cabi.GQError(f"sample_logits: rows overlap (row stride {ld} < V={V})")
    if not 1 <= int(top_k) <= SAMPLE_MAX_K:
        raise _cabi.GQError(f"sample_logits: top_k={top_k} (not in [1, {SAMPLE_MAX_K}]; an unbounded nucleus is not built)")
    if u is None:
        if temperature != 0:
            raise _cabi.GQError(f"sample_logits: u is None with temperature={temperature} (only the argmax needs no draw)")
    elif u.dtype != torch.float32 or u.numel() != B or u.device != logits.device:
        raise _cabi.GQError(f"sample_logits: u must be fp32 [{B}] on {logits.device}; got {u.dtype} {tuple(u.shape)} on "
                            f"{u.device}")
    else:
        u = u.contiguous()
    ids = torch.empty(B, dtype=torch.int64, device=logits.device)
    check(lib().gq_sample_logits(_ptr(logits), _DT[logits.dtype], B, V, ld, int(top_k), float(top_p), float(temperature),
                                 _ptr(u), _ptr(ids), _stream(logits)), "gq_sample_logits")
    return ids
