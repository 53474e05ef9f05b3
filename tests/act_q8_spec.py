"""include/gptq_gguf_qgemm_a8.h restated in numpy: the activation quantizer operation by operation in fp32 (byte for byte the
kernel's outputs) and the terms of gq_linear_packed_a8 in fp64 from exact integers, with the sums its error bound is made of.
The weight side comes from ggml_spec.unpack and ggml_spec's Q8_0 layout."""
import numpy as np

from ggml_spec import unpack

Q8_0 = 8
f32 = np.float32


def quantize(x):
    """x: float32 [T, C] holding fp16- or bf16-representable values -> (xq int8 [T, C], xd float32 [T, C/256], xbsum int16 [T, C/16])."""
    T, C = x.shape
    b = np.asarray(x, f32).reshape(T, C // 256, 256)
    amax = np.abs(b).max(axis=2)
    with np.errstate(divide="ignore"):
        inv = f32(127) / amax
    d = amax / f32(127)
    zero = (amax == 0) | ~np.isfinite(inv)
    inv, d = np.where(zero, f32(0), inv).astype(f32), np.where(zero, f32(0), d).astype(f32)
    q = np.clip(np.rint(b * inv[..., None]), -127, 127).astype(np.int8)  # (np.rint: ties to even)
    return q.reshape(T, C), d, q.reshape(T, C // 16, 16).astype(np.int32).sum(axis=2).astype(np.int16)


def _h(bits):
    return np.ascontiguousarray(bits).astype(np.uint16).view(np.float16).astype(np.float64)


def terms(q_type, packed, xq, xd, xbsum):
    """packed uint8 [R, row bytes] -> (ref, mag) float64 [T, R]: ref = sum_j term_j exactly, mag = sum_j (|xd d isum_j| +
    |xd dmin msum_j|) (Q8_0: sum_j sum_b |xd d_b isum_b|), the magnitude that the fp32 roundings of the contract scale with."""
    T, C = xq.shape
    R, nsb = packed.shape[0], C // 256
    xi, xdd = xq.astype(np.int64), xd.astype(np.float64)
    if q_type == Q8_0:
        blk = packed.reshape(R, C // 32, 34)
        d = _h(blk[:, :, 0].astype(np.uint16) | (blk[:, :, 1].astype(np.uint16) << 8))        # [R, C/32]
        w = blk[:, :, 2:].copy().view(np.int8).astype(np.int64)                                # [R, C/32, 32]
        isum = np.einsum("tbk,rbk->trb", xi.reshape(T, C // 32, 32), w)                        # exact
        part = isum * d[None] * np.repeat(xdd, 8, axis=1)[:, None, :]
        return part.sum(axis=2), np.abs(part).sum(axis=2)
    codes, d, sc, dmin, mn = unpack(q_type, packed)
    G = C // sc.shape[1]
    gs = np.einsum("tgk,rgk->trg", xi.reshape(T, C // G, G), codes.astype(np.int64).reshape(R, C // G, G))
    isum = (gs * sc[None].astype(np.int64)).reshape(T, R, nsb, -1).sum(axis=3)
    bs = xbsum.astype(np.int64).reshape(T, C // G, G // 16).sum(axis=2)                        # the sums of the type's groups
    msum = (bs[:, None, :] * mn[None].astype(np.int64)).reshape(T, R, nsb, -1).sum(axis=3)
    a, b = xdd[:, None, :] * _h(d)[None] * isum, xdd[:, None, :] * _h(dmin)[None] * msum
    return (a - b).sum(axis=2), (np.abs(a) + np.abs(b)).sum(axis=2)


def decode64(q_type, packed, C):
    """The exact fp64 weight [R, C] of the packed rows."""
    R = packed.shape[0]
    if q_type == Q8_0:
        blk = packed.reshape(R, C // 32, 34)
        d = _h(blk[:, :, 0].astype(np.uint16) | (blk[:, :, 1].astype(np.uint16) << 8))
        return (blk[:, :, 2:].copy().view(np.int8).astype(np.float64) * d[:, :, None]).reshape(R, C)
    codes, d, sc, dmin, mn = unpack(q_type, packed)
    G = C // sc.shape[1]
    rep = lambda v, n: np.repeat(v, n, axis=1)  # noqa: E731
    return rep(_h(d), 256) * rep(sc, G) * codes - rep(_h(dmin), 256) * rep(mn, G)
