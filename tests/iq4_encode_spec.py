"""The IQ4_NL / IQ4_XS encoder as include/gptq_gguf_iq4_encode.h states it, restated element by element in np.float32 scalars:
loops over super-blocks, blocks and j, one operation at a time, every sum in ascending j.  Nothing is shared with
gguf_writer.quantize_iq4 (the vectorised host form) or with the kernel: tests/test_iq4_encode_cpu.py compares the host form with
these loops byte for byte, tests/test_gpu_iq4_encode.py the kernel with the host form.  The module also holds the inputs both
test files share (crafted blocks, the generators)."""
import numpy as np

NL, XS = 20, 23
GEOMETRY = {NL: (32, 18), XS: (256, 136)}
KV = (-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113)
F = np.float32
KVF = tuple(F(v) for v in KV)


def best(a):
    """The index of the table entry nearest to the fp32 `a`; the two ROUNDED differences are compared, a tie goes up."""
    a = F(a)
    if a <= KVF[0]:
        return 0
    if a >= KVF[15]:
        return 15
    u = 1
    while not KVF[u] > a:
        u += 1
    return u - 1 if F(a - KVF[u - 1]) < F(KVF[u] - a) else u


def sums(x, w, id_):
    sumqx, sumq2 = F(0), F(0)
    for j in range(32):
        q = KVF[best(F(id_ * x[j]))]
        wq = F(w[j] * q)
        sumqx = F(sumqx + F(wq * x[j]))
        sumq2 = F(sumq2 + F(wq * q))
    return sumqx, sumq2


def block_scale(x, w):
    """The scale d of one 32-value block x (fp32) under the weights w."""
    amax, mx = F(0), F(0)
    for j in range(32):
        ax = F(abs(x[j]))
        if ax > amax:
            amax, mx = ax, x[j]
    if amax < F(1e-15):
        return F(0)
    d0 = F(F(-mx) / KVF[0])
    sumqx, sumq2 = sums(x, w, F(F(1) / d0))
    d = F(sumqx / sumq2)
    bst = F(d * sumqx)
    for itry in range(-7, 8):
        id_ = F(F(F(itry) + KVF[0]) / mx)
        sumqx, sumq2 = sums(x, w, id_)
        if sumq2 > 0 and F(sumqx * sumqx) > F(bst * sumq2):
            d = F(sumqx / sumq2)
            bst = F(d * sumqx)
    return d


def half_bytes(v):
    return np.array([v], np.float32).astype(np.float16).tobytes()  # round-to-nearest-even


def encode_superblock(t, x, imp):
    """x: the super-block's values, fp32 (256 for XS, 32 for NL); imp: its importance values or None -> bytes."""
    size = GEOMETRY[t][0]
    s = F(0)
    for j in range(size):
        s = F(s + F(x[j] * x[j]))
    sigma2 = F(s * F(F(2) / F(size)))
    ds = []
    for ib in range(size // 32):
        xb = x[32 * ib:32 * ib + 32]
        use = imp is not None and any(imp[32 * ib + j] != 0 for j in range(32))
        w = []
        for j in range(32):
            x2 = F(xb[j] * xb[j])
            w.append(F(imp[32 * ib + j] * np.sqrt(F(sigma2 + x2), dtype=np.float32)) if use else x2)
        ds.append(block_scale(xb, w))

    def codes(xb, idl):
        L = [best(F(idl * xb[j])) for j in range(32)]
        return bytes(L[j] | (L[j + 16] << 4) for j in range(16))

    if t == NL:
        d = ds[0]
        return half_bytes(d) + codes(x, F(F(1) / d) if d != 0 else F(0))
    amax, ms = F(0), F(0)
    for d in ds:
        if F(abs(d)) > amax:
            amax, ms = F(abs(d)), d
    D = F(F(-ms) / F(32))
    iD = F(F(1) / D) if D != 0 else F(0)
    scales_h, scales_l, qs = 0, [0, 0, 0, 0], b""
    for ib in range(8):
        l = int(max(-32, min(31, np.rint(F(iD * ds[ib])))))
        dl = F(D * F(l))
        qs += codes(x[32 * ib:32 * ib + 32], F(F(1) / dl) if dl != 0 else F(0))
        ls = l + 32
        scales_l[ib // 2] |= (ls & 15) << (4 * (ib % 2))
        scales_h |= (ls >> 4) << (2 * ib)
    return half_bytes(D) + bytes([scales_h & 255, scales_h >> 8, *scales_l]) + qs


def encode(t, x, importance=None):
    """x float32 [R, C] -> uint8 [R, C / block * bytes]."""
    x = np.ascontiguousarray(x, np.float32)
    R, C = x.shape
    bs, ts = GEOMETRY[t]
    assert C % bs == 0
    imp = None if importance is None else np.ascontiguousarray(importance, np.float32)
    out = bytearray()
    with np.errstate(all="ignore"):
        for r in range(R):
            for sb in range(C // bs):
                out += encode_superblock(t, x[r, bs * sb:bs * sb + bs], None if imp is None else imp[bs * sb:bs * sb + bs])
    return np.frombuffer(bytes(out), np.uint8).reshape(R, C // bs * ts)


# ---------------------------------------------------------------------------------------------------------------- inputs
def random_matrix(R, C, seed):
    return (np.random.default_rng(seed).standard_normal((R, C)) * 0.03).astype(np.float32)


def random_importance(C, seed):
    return (10 * np.random.default_rng(1000 + seed).random(C) ** 4 + 1e-3).astype(np.float32)


def honest_case(seed):
    """The generator of the two conditions that keep the encoder honest: x = 0.03 N(0, 1) fp32 [33, 768] with 1 % of the entries
    times 6, qw = 10 U^4 + 1e-3."""
    rng = np.random.default_rng(seed)
    x = (0.03 * rng.standard_normal((33, 768))).astype(np.float32)
    x[rng.random(x.shape) < 0.01] *= np.float32(6)
    qw = (10 * rng.random(768) ** 4 + 1e-3).astype(np.float32)
    return x, qw


def crafted(t):
    """(x [R, C] fp32, importance [C]) of the crafted blocks.  C is 512 for XS (two super-blocks a row) and 64 for NL; every row
    starts as 0.03 N(0, 1) and gets one feature:
      0  all zero                              1  amax = 1e-20 (every block of the row: the scale is 0)
      2  +m before -m, tied for amax           3  -m before +m
      4  one block 100 x the others (XS: l = -32 for it, l = 0 for some)
      5  ordinary values under the zero importance of columns 32 .. 63
      6  values that land exactly on table entries after scaling: max = -127 * 2^-12 and x = kv * 2^-12 elsewhere, so the
         candidate itry = 0, id = 2^12, maps them onto the table itself (and onto midpoints of it: (kv[a] + kv[b]) / 2 * 2^-12)"""
    C = 512 if t == XS else 64
    rng = np.random.default_rng(7 + t)
    x = (0.03 * rng.standard_normal((7, C))).astype(np.float32)
    imp = (10 * rng.random(C) ** 4 + 1e-3).astype(np.float32)
    imp[32:64] = 0
    x[0] = 0
    x[1] = np.float32(1e-20) * np.sign(x[1])
    m = np.float32(0.2)
    x[2, 5], x[2, 20] = m, -m
    x[3, 5], x[3, 20] = -m, m
    x[4] *= np.float32(0.01)
    x[4, 64 % C:64 % C + 32] *= np.float32(100)
    k = np.array(KV, np.float32)
    step = np.float32(2.0 ** -12)
    x[6, :16] = k * step
    x[6, 16:31] = (k[:-1] + k[1:]) / 2 * step
    x[6, 31] = 0
    return x, imp


def xs_scales(blocks):
    """Every ls of IQ4_XS blocks uint8 [..., n * 136] -> int array [nblocks, 8]."""
    b = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 136)
    sh = b[:, 2].astype(np.int64) | (b[:, 3].astype(np.int64) << 8)
    return np.stack([((b[:, 4 + ib // 2] >> (4 * (ib % 2))) & 15) | (((sh >> (2 * ib)) & 3) << 4) for ib in range(8)], 1)
