"""The grouped MoE kernels at real expert counts: the stacked weights, the named pair sets, the scalar restatement of
linear_packed_experts_kernel's tile lookup and the vectorised references tests/test_gpu_moe_experts.py compares against.  A plain
helper, no test; tests/test_moe_cases_cpu.py pins on the host what the GPU tests rely on.

    stacked(ops, t, E, R, C)                          the packed [E, R, C] tensor of type t on the device, made once per key
    inputs(x_rows, C, dt, t)                          the seeded activations
    PAIR_SETS[name]()                                 -> (x_rows, pairs_per_row, ids), seeded
    EXPECT[name]                                      E, the tile width, the tile count and the (lane, k) slots of the set
    tile_of(b, expert_start, TT)                      the (expert, first position, tokens) of workgroup tile b, or None
    lane_k(e)                                         the lane and the slot of expert e in the kernel's wave-wide search
    expected_rows(ops, t, src, E, ids, x, ppr)        -> (want [P, R], written [P]): ops.linear_packed per named expert
    gemv_rows(ops, t, src, E, ids, x, ppr)            -> (want [P, R], written [P]): ops.gemv_packed per named pair
    fp64_rows(ops, t, src, E, R, C, ids, x, ppr, dt)  -> (y64 [P, R], bound [P, R])
    routing, composed_decode, composed_prefill, fp64_and_bound   the module-level references, for any E and K

The kernel's search (csrc/qgemm/gq_moe_gemm.hip): lane l holds the starts of experts 4 l .. 4 l + 3 and one more, read at
min(e, E); the lanes' tile counts are prefix-summed, a ballot picks the lane whose range holds tile b, that lane walks its four
experts and its answer is broadcast.  With E <= 4 everything is lane 0's; the sets below put tiles into the other lanes."""
import torch

Q2, Q3, Q4, Q5, Q6, Q8, NL, XS = 10, 11, 12, 13, 14, 8, 20, 23
ALL8 = (Q2, Q3, Q4, Q5, Q6, Q8, NL, XS)
WIDE_OK = (Q2, Q3, Q6, Q8, NL)  # the types with a 256-token instance of the grouped GEMM; the others keep 128 tokens at any size
F16, BF16 = torch.float16, torch.bfloat16
PER = 4  # experts per lane

_cache = {}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ weights and activations
def stacked(ops, t, E, R, C):
    """The packed [E, R, C] tensor of one type and shape as a 1-D uint8 view at a 16-byte aligned address: quantized once,
    shared by every test.  K-quants and Q8_0: test_gpu_qgemm.packed_weight (seeded N(0, 0.02^2): every decode is finite);
    IQ4_NL / IQ4_XS: iq4_spec.gemm_fixture (|d| in [2^-10, 2^-1)).  E > 256: the bytes of 4 distinct experts repeated
    (expert e holds the bytes of e % 4): block bytes do not depend on their position."""
    key = (t, E, R, C)
    if key not in _cache:
        n = min(E, 4) if E > 256 else E
        if t in (NL, XS):
            import iq4_spec
            import numpy as np
            src = torch.from_numpy(np.ascontiguousarray(iq4_spec.gemm_fixture(t, n * R, C))).reshape(-1).cuda()
        else:
            from test_gpu_qgemm import packed_weight
            src, _ = packed_weight(ops, t, n * R, C, seed=7000 + t + R + C + E, scale=0.02)
        if n != E:
            src = src.view(n, -1)[torch.arange(E, device="cuda") % n].reshape(-1)
        assert src.is_contiguous() and src.data_ptr() % 16 == 0
        _cache[key] = src
    return _cache[key]


def inputs(x_rows, C, dt, t=Q4):
    """Seeded N(0, 1) activations; N(0, 2^-6) for IQ4_XS, whose fixture decodes to weights of up to 1968 in magnitude: a row
    of 512 of them times N(0, 1) comes within a few sigma of fp16's largest value."""
    x = torch.randn(x_rows, C, generator=_gen(x_rows + C))
    return (x * 0.125 if t == XS else x).to(dt).cuda()


# ------------------------------------------------------------------------------------------------ the pair sets
def _shuffled(ids, seed):
    return [ids[i] for i in torch.randperm(len(ids), generator=_gen(seed)).tolist()]


def _by_counts(counts, seed, masked=0):
    """`counts[e]` pairs of expert e and `masked` ids of -1, in a seeded order."""
    return _shuffled([e for e, c in sorted(counts.items()) for _ in range(c)] + [-1] * masked, seed)


def _top_k(T, E, K, seed):
    """The row-major [T, K] index of the top-K of random logits: distinct experts per token."""
    return torch.topk(torch.randn(T, E, generator=_gen(seed)), K, -1).indices.reshape(-1).tolist()


SKEWED8 = {0: 42, 1: 129, 5: 128, 6: 400, 7: 1}
WIDE8 = {0: 16, 2: 257, 4: 17, 5: 600, 7: 256}
WIDE9 = {0: 595, 3: 256, 4: 1, 8: 300}


def _masked8():
    ids = _by_counts(SKEWED8, 22)
    for i, p in enumerate(torch.randperm(700, generator=_gen(28)).tolist()[:60]):
        ids[p] = (-1, 8, 2 ** 30)[i % 3]
    return 700, 1, ids


def _switch(P):
    """P ids drawn from wide8's distribution, the -1 included."""
    pool = _by_counts(WIDE8, 29, masked=134)
    return P, 1, [pool[i] for i in torch.randint(0, len(pool), (P,), generator=_gen(P)).tolist()]


PAIR_SETS = {
    # the 128-token tile
    "mixtral": lambda: (150, 2, _top_k(150, 8, 2, 21)),
    "skewed8": lambda: (700, 1, _by_counts(SKEWED8, 22)),
    "tiny5": lambda: (40, 2, _top_k(40, 5, 2, 23)),
    "qwen64": lambda: (33, 8, _top_k(33, 64, 8, 24)),
    "each256": lambda: (256, 1, torch.randperm(256, generator=_gen(25)).tolist()),
    "last256": lambda: (130, 1, [255] * 130),
    "last255": lambda: (130, 1, [254] * 130),
    "masked8": _masked8,
    "switch1023": lambda: _switch(1023),
    # the 256-token tile (the types of WIDE_OK; the others run these with 128 tokens)
    "wide8": lambda: (160, 8, _by_counts(WIDE8, 26, masked=134)),
    "wide9": lambda: (1152, 1, _by_counts(WIDE9, 27)),
    "switch1024": lambda: _switch(1024),
}

_slots = lambda experts: {(e // PER, e % PER) for e in experts}  # noqa: E731
# name -> E, whether P >= 128 E, the number of tiles at the set's own width (128 narrow, 256 wide; None: whatever the seeded draw
# gives, one per named expert at least), the (lane, k) slots that hold a tile, or the lanes where the draw decides the slots
EXPECT = {
    "mixtral": dict(E=8, wide=False, tiles=8, slots=_slots(range(8))),
    "skewed8": dict(E=8, wide=False, tiles=9, slots=_slots(SKEWED8)),
    "tiny5": dict(E=5, wide=False, tiles=5, slots=_slots(range(5))),
    "qwen64": dict(E=64, wide=False, tiles=None, lanes=set(range(16))),
    "each256": dict(E=256, wide=False, tiles=256, slots=_slots(range(256))),
    "last256": dict(E=256, wide=False, tiles=2, slots={(63, 3)}),
    "last255": dict(E=255, wide=False, tiles=2, slots={(63, 2)}),
    "masked8": dict(E=8, wide=False, tiles=None, slots=_slots(SKEWED8)),
    "switch1023": dict(E=8, wide=False, tiles=None, slots=_slots(WIDE8)),
    "wide8": dict(E=8, wide=True, tiles=8, slots=_slots(WIDE8)),
    "wide9": dict(E=9, wide=True, tiles=7, slots=_slots(WIDE9)),
    "switch1024": dict(E=8, wide=True, tiles=None, slots=_slots(WIDE8)),
}
NARROW = [n for n in PAIR_SETS if not EXPECT[n]["wide"] and not n.startswith("switch")]
SMALL = [n for n in NARROW if EXPECT[n]["E"] < 255]
MANY = [n for n in NARROW if EXPECT[n]["E"] >= 255]

# the (set, type, dtype) cases of the grouped GEMM: four types per small narrow set, two per 255 / 256-expert set (a 16-byte
# aligned K-quant and IQ4_NL), seven per wide set with the dtype swapped between the two -- test_moe_cases_cpu.py checks that every
# type meets both dtypes
GEMM_NARROW = ([(n, ALL8[(i + 2 * j) % 8], (F16, BF16)[(i + j) % 2]) for i, n in enumerate(SMALL) for j in range(4)] +
               [(n, t, (F16, BF16)[(i + j) % 2]) for i, n in enumerate(MANY) for j, t in enumerate((Q4, NL))])
GEMM_WIDE = [(n, t, (F16, BF16)[(i + j) % 2]) for i, n in enumerate(("wide8", "wide9")) for j, t in enumerate(WIDE_OK + (Q4, XS))]


def grid_tiles(P, E, TT):
    """The host's second grid dimension: an upper bound of the number of tiles that needs no count."""
    return (P + TT - 1) // TT + min(E, P)


def tile_of(b, expert_start, TT):
    """Workgroup tile b of a route: (expert, first position in `order`, tokens), or None when the runs have fewer tiles.  The
    tiles of expert 0 come first, then expert 1's, ...; an empty expert has none."""
    for e in range(len(expert_start) - 1):
        n = -(-(expert_start[e + 1] - expert_start[e]) // TT)
        if b < n:
            pos0 = expert_start[e] + b * TT
            return e, pos0, min(TT, expert_start[e + 1] - pos0)
        b -= n
    return None


def lane_k(e):
    """(lane, slot) of expert e in the kernel's search."""
    return e // PER, e % PER


# ------------------------------------------------------------------------------------------------ the kernel references
def _named(ids, E):
    """{expert: the indices of the pairs that name it, ascending}."""
    runs = {}
    for p, e in enumerate(ids):
        if 0 <= e < E:
            runs.setdefault(e, []).append(p)
    return runs


def expected_rows(ops, t, src, E, ids, x, ppr):
    """(want [P, R], written [P] bool): the contract's reference -- per named expert ONE ops.linear_packed call on that expert's
    slice with its gathered tokens, scattered to pair order.  A row of a pair that names no expert is zero and not `written`."""
    slices = src.view(E, -1)
    P = len(ids)
    want, written = None, torch.zeros(P, dtype=torch.bool)
    for e, mine in sorted(_named(ids, E).items()):
        at = torch.tensor(mine)
        y = ops.linear_packed(t, slices[e], x[(at // ppr).cuda()].contiguous())
        if want is None:
            want = torch.zeros(P, y.shape[1], dtype=x.dtype, device="cuda")
        want[at.cuda()] = y
        written[at] = True
    return want, written.cuda()


def gemv_rows(ops, t, src, E, ids, x, ppr):
    """The same for the grouped GEMV, as its header words it: row p is ops.gemv_packed of the expert's slice and the one row
    x[p // ppr]."""
    slices = src.view(E, -1)
    rows, written = [], []
    for p, e in enumerate(ids):
        written.append(0 <= e < E)
        rows.append(ops.gemv_packed(t, slices[e], x[p // ppr:p // ppr + 1])[0] if written[-1] else None)
    zero = torch.zeros_like(next(r for r in rows if r is not None))
    return torch.stack([zero if r is None else r for r in rows]), torch.tensor(written).cuda()


def fp64_rows(ops, t, src, E, R, C, ids, x, ppr, dt):
    """(y64 [P, R], bound [P, R]) per named expert, test_gpu_qgemm.py's bound unchanged: u |y64| + C 2^-23 (|x| |Wd|^T) + 2^-25
    per element, u = 2^-11 (fp16) or 2^-8 (bf16) -- the final rounding plus the worst-case fp32 accumulation of C terms in any
    order; Wd is the block decoder's weight in the operand dtype.  Derived, not measured.  Rows of unnamed pairs are zero."""
    u = 2.0 ** -11 if dt == F16 else 2.0 ** -8
    Wd = ops.dequantize_blocks(t, src.view(E * R, -1), dt).view(E, R, C)
    y64 = torch.zeros(len(ids), R, dtype=torch.float64, device="cuda")
    bound = torch.zeros_like(y64)
    for e, mine in sorted(_named(ids, E).items()):
        at = torch.tensor(mine).cuda()
        xe, We = x[at // ppr].double(), Wd[e].double()
        y = xe @ We.T
        y64[at] = y
        bound[at] = u * y.abs() + C * 2.0 ** -23 * (xe.abs() @ We.abs().T) + 2.0 ** -25
    return y64, bound


# ------------------------------------------------------------------------------------------------ the module references
ROLES = ("gate", "up", "down")


def routing(T, E, K, seed):
    """Top-K of random logits, distinct experts per token, the weights normalised: (index [T, K], weights [T, K]) on the device."""
    w, idx = torch.topk(torch.softmax(torch.randn(T, E, generator=_gen(seed)), -1), K, -1)
    return idx.cuda(), (w / w.sum(-1, keepdim=True)).cuda()


def _slices(ex):
    return {r: (ex.levels[r][0].view(ex.num_experts, -1), ex.levels[r][1]) for r in ROLES}


def composed_decode(ex, x, idx, w):
    """The decode path spelled out (test_gpu_moe_model.py's `composed`, E and K from the module and the index): per pair
    ops.gemv_packed on the expert's slices, fwd_silu_mul, then the fp32 sum over k ascending and one rounding.  A pair whose id
    is outside [0, E) adds zero."""
    from gptq_gguf_toolkit_amd import ops
    sl, E = _slices(ex), ex.num_experts
    ids, rows = idx.tolist(), []
    for t in range(x.shape[0]):
        acc = None
        for k, e in enumerate(ids[t]):
            if 0 <= e < E:
                a = ops.fwd_silu_mul(ops.gemv_packed(sl["gate"][1], sl["gate"][0][e], x[t:t + 1]),
                                     ops.gemv_packed(sl["up"][1], sl["up"][0][e], x[t:t + 1]))
                term = ops.gemv_packed(sl["down"][1], sl["down"][0][e], a).float() * w[t, k].float()
            else:
                term = torch.zeros(1, ex.hidden_dim, device="cuda")
            acc = term if acc is None else acc + term
        rows.append(acc)
    return torch.cat(rows).to(x.dtype)


def composed_prefill(ex, x, idx, w):
    """The grouped prefill spelled out (test_gpu_moe_prefill_model.py's `composed`, E and K from the module and the index):
    ops.moe_route, per expert ops.linear_packed on the slices of the three stacked tensors with the expert's tokens gathered by
    the route, ops.fwd_silu_mul, and the combine the decode path shares."""
    from gptq_gguf_toolkit_amd import ops
    sl, E, H, I = _slices(ex), ex.num_experts, ex.hidden_dim, ex.intermediate_dim
    T, K = idx.shape
    pairs = idx.reshape(-1).to(torch.int32)
    start, order = ops.moe_route(pairs, E)
    start = start.tolist()
    gate, up = (torch.zeros(T * K, I, dtype=x.dtype, device="cuda") for _ in range(2))
    down = torch.full((T * K, H), float("nan"), dtype=x.dtype, device="cuda")
    runs = [order[start[e]:start[e + 1]].long() for e in range(E)]
    for e, run in enumerate(runs):
        if run.numel():
            cur = x[run // K].contiguous()
            gate[run] = ops.linear_packed(sl["gate"][1], sl["gate"][0][e], cur)
            up[run] = ops.linear_packed(sl["up"][1], sl["up"][0][e], cur)
    a = ops.fwd_silu_mul(gate, up)
    for e, run in enumerate(runs):
        if run.numel():
            down[run] = ops.linear_packed(sl["down"][1], sl["down"][0][e], a[run].contiguous())
    return ex._combine(down, pairs, w)


def fp64_and_bound(ex, x, idx, w):
    """out64 and B with |out - out64| <= B for every path of the module: test_gpu_moe_model.py's `fp64_and_bound` for any K and
    for bf16 (u = 2^-11 fp16, 2^-8 bf16), all in fp64 on the weights decoded to the module's dtype.  With b(y) = u |y64| +
    C 2^-23 (|x| |W|^T) + 2^-25 the one-Linear bound of test_gpu_qgemm.py (final rounding + fp32 accumulation of C terms):
      gate, up:  |g^ - g| <= b_g, |u^ - u| <= b_u                                   (one Linear each, C = H)
      a = silu(g) u:  silu is 1.1-Lipschitz, so |silu(g^) u^ - a| <= 1.1 b_g (|u| + b_u) + |silu(g)| b_u =: p; the product is
                 rounded once (the fused kernel): <= 2u (|a| + p) more, plus 2^-20 |a| for the device exp -> b_a
      down:      |d^ - d| <= (b_a |Wd|^T) + u (|d| + b_a |Wd|^T) + I 2^-23 ((|a| + b_a) |Wd|^T) + 2^-25 =: b_d
      sum:       sum_k w_k d_k.  The decode and the prefill path add K terms in fp32 and round once.  The loop path rounds each
                 of the K products w_k d_k to 16 bits, u |term_k| each, and then makes K - 1 additions in 16 bits (index_add_),
                 each at most u times a partial sum, and a partial sum is <= sum_k |term_k|: K u sum_k |term_k| plus second-order
                 terms in all.  (K + 1) u sum_k (|w_k d_k| + w_k b_d,k) covers it; at K = 2 this is the 3u of the K = 2 file.
    B = sum_k w_k b_d,k + (K + 1) u sum_k (|w_k d_k| + w_k b_d,k).  A pair whose id is outside [0, E) has no term.  Derived, not
    measured."""
    u = 2.0 ** -11 if x.dtype == F16 else 2.0 ** -8
    E, H, I = ex.num_experts, ex.hidden_dim, ex.intermediate_dim
    K = idx.shape[1]
    Wg, Wu, Wd = (ex.dense_weight(r).double() for r in ROLES)
    xd = x.double()
    out = torch.zeros(x.shape[0], H, dtype=torch.float64, device="cuda")
    B = torch.zeros_like(out)
    mag = torch.zeros_like(out)
    ids, ws = idx.tolist(), w.tolist()
    for t in range(x.shape[0]):
        for k in range(K):
            e, wk = ids[t][k], ws[t][k]
            if not 0 <= e < E:
                continue
            g, up = Wg[e] @ xd[t], Wu[e] @ xd[t]
            b_g = u * g.abs() + H * 2.0 ** -23 * (Wg[e].abs() @ xd[t].abs()) + 2.0 ** -25
            b_u = u * up.abs() + H * 2.0 ** -23 * (Wu[e].abs() @ xd[t].abs()) + 2.0 ** -25
            s = torch.nn.functional.silu(g)
            a = s * up
            p = 1.1 * b_g * (up.abs() + b_u) + s.abs() * b_u
            b_a = p + 2 * u * (a.abs() + p) + 2.0 ** -20 * a.abs()
            d = Wd[e] @ a
            carried = Wd[e].abs() @ b_a
            b_d = carried + u * (d.abs() + carried) + I * 2.0 ** -23 * (Wd[e].abs() @ (a.abs() + b_a)) + 2.0 ** -25
            out[t] += wk * d
            B[t] += wk * b_d
            mag[t] += wk * (d.abs() + b_d)
    return out, B + (K + 1) * u * mag
