"""IQ4_NL and IQ4_XS as include/gptq_gguf_iq4.h states them, restated element by element (ggml's dequantize_row_iq4_nl /
dequantize_row_iq4_xs: a loop over blocks, sub-blocks ib and bytes j, one value at a time), and the block fixtures the IQ4 tests
share: tests/test_iq4_cpu.py pins them on the host, tests/test_gpu_iq4.py runs them on the GPU.

Arithmetic: d * (ls - 32) * kv is exact in fp32 (11 + 6 + 7 significant bits), hence also in the Python floats the loops use;
storing into a float32 array changes nothing.  inf * 0 is NaN in both."""
import numpy as np

import gguf_spec_writer

NL, XS = 20, 23                       # the ggml type ids
GEOMETRY = {NL: (32, 18), XS: (256, 136)}   # (values, bytes) per block
NAME = {NL: "IQ4_NL", XS: "IQ4_XS"}
KV = (-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113)

# tests/gguf_spec_writer.py serialises by type name from these two tables; the two names are added, nothing else changes
for _t in (NL, XS):
    gguf_spec_writer.GGML.setdefault(NAME[_t], _t)
    gguf_spec_writer.BLOCK.setdefault(NAME[_t], GEOMETRY[_t])


def _half(lo, hi):
    """The value of the fp16 whose bytes are lo, hi, as a Python float."""
    return float(np.array([lo | (hi << 8)], np.uint16).view(np.float16)[0])


def decode_iq4_nl(raw, n):
    """raw: n / 32 blocks { fp16 d; uint8 qs[16]; } -> float32 [n]."""
    raw = bytes(raw)
    assert n % 32 == 0 and len(raw) == n // 32 * 18
    y = np.empty(n, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(n // 32):
            blk = raw[18 * b:18 * b + 18]
            d = _half(blk[0], blk[1])
            for j in range(16):
                q = blk[2 + j]
                y[32 * b + j] = d * KV[q & 15]
                y[32 * b + j + 16] = d * KV[q >> 4]
    return y


def xs_scale(blk, ib):
    """ls of sub-block ib of one 136-byte superblock, 0 .. 63."""
    scales_h = blk[2] | (blk[3] << 8)
    return ((blk[4 + ib // 2] >> (4 * (ib % 2))) & 15) | (((scales_h >> (2 * ib)) & 3) << 4)


def decode_iq4_xs(raw, n):
    """raw: n / 256 superblocks { fp16 d; uint16 scales_h; uint8 scales_l[4]; uint8 qs[128]; } -> float32 [n]."""
    raw = bytes(raw)
    assert n % 256 == 0 and len(raw) == n // 256 * 136
    y = np.empty(n, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(n // 256):
            blk = raw[136 * b:136 * b + 136]
            d = _half(blk[0], blk[1])
            for ib in range(8):
                dl = d * (xs_scale(blk, ib) - 32)
                for j in range(16):
                    q = blk[8 + 16 * ib + j]
                    y[256 * b + 32 * ib + j] = dl * KV[q & 15]
                    y[256 * b + 32 * ib + 16 + j] = dl * KV[q >> 4]
    return y


def decode(t, blocks):
    """uint8 [R, C / block * bytes] (or [E, R, ...]: any leading shape) -> float32 [..., C]."""
    blocks = np.ascontiguousarray(blocks, np.uint8)
    bs, ts = GEOMETRY[t]
    assert blocks.shape[-1] % ts == 0
    n = blocks.size // ts * bs
    y = (decode_iq4_nl if t == NL else decode_iq4_xs)(blocks.tobytes(), n)
    return y.reshape(*blocks.shape[:-1], blocks.shape[-1] // ts * bs)


# ---------------------------------------------------------------------------------------------------------------- builders
def nl_block(d_bits, qs):
    """One IQ4_NL block from its fields: d as fp16 bits, qs 16 bytes."""
    assert len(qs) == 16
    return bytes([d_bits & 255, d_bits >> 8, *qs])


def xs_block(d_bits, scales_h, scales_l, qs):
    """One IQ4_XS superblock from its fields: d as fp16 bits, scales_h 16 bits, scales_l 4 bytes, qs 128 bytes."""
    assert len(scales_l) == 4 and len(qs) == 128
    return bytes([d_bits & 255, d_bits >> 8, scales_h & 255, scales_h >> 8, *scales_l, *qs])


def finite_d_bits(rng, n):
    """n fp16 bit patterns drawn from ALL finite values of both signs (exponent 31 -> 30), every seventh one an fp16
    subnormal (exponent 0)."""
    bits = rng.integers(0, 1 << 16, size=n, dtype=np.uint16)
    bits[(bits & 0x7C00) == 0x7C00] &= 0xFBFF
    bits[::7] &= 0x83FF
    return bits


def gemm_d_bits(rng, n):
    """n fp16 bit patterns with |d| in [2^-10, 2^-1) and a random sign: exponent field 5 .. 13, any mantissa."""
    e = rng.integers(5, 14, size=n, dtype=np.uint16)
    m = rng.integers(0, 1 << 10, size=n, dtype=np.uint16)
    s = rng.integers(0, 2, size=n, dtype=np.uint16)
    return (s << 15) | (e << 10) | m


def model_d_bits(exponent):
    """|d| in [2^(exponent - 15), 2^(exponent - 14)) and a random sign."""
    def draw(rng, n):
        return ((rng.integers(0, 2, size=n, dtype=np.uint16) << 15) | (np.uint16(exponent) << 10) |
                rng.integers(0, 1 << 10, size=n, dtype=np.uint16))
    return draw


def blocks_with_d(t, R, C, seed, d_bits=finite_d_bits):
    """uint8 [R, C / block * bytes]: d from `d_bits`, every other byte uniform."""
    bs, ts = GEOMETRY[t]
    assert C % bs == 0
    rng = np.random.default_rng(seed)
    nb = R * C // bs
    b = rng.integers(0, 256, size=(nb, ts), dtype=np.uint8)
    b[:, :2] = d_bits(rng, nb).astype("<u2").view(np.uint8).reshape(nb, 2)
    return b.reshape(R, C // bs * ts)


def with_inf_block(t, blocks, at=1):
    """A copy with d = +inf in block `at` (flat index); for IQ4_XS its sub-block 0 gets ls = 32 (inf * 0 = NaN) and its
    sub-block 1 ls = 33."""
    bs, ts = GEOMETRY[t]
    out = blocks.copy()
    b = out.reshape(-1, ts)
    b[at, 0], b[at, 1] = 0x00, 0x7C
    if t == XS:
        b[at, 2] = (b[at, 2] & 0xF0) | 0b1010       # the high two bits of ls 0 and ls 1: 2, 2
        b[at, 4] = 0x10                               # the low nibbles: 0, 1
    return out


def model_blocks(t, R, C, seed):
    """Blocks that decode to weights a small model can run with, about 0.03 rms and none an fp16 subnormal: IQ4_XS with |d| in
    [2^-14, 2^-13) and |ls - 32| <= 8, IQ4_NL with |d| in [2^-12, 2^-11) (kv has an rms of 68)."""
    out = blocks_with_d(t, R, C, seed, model_d_bits(1 if t == XS else 3))
    if t == XS:
        rng = np.random.default_rng(seed + 1)
        b = out.reshape(-1, 136)
        ls = rng.integers(24, 41, size=(b.shape[0], 8), dtype=np.uint16)
        b[:, 2:4] = sum((ls[:, i] >> 4) << (2 * i) for i in range(8)).astype("<u2").view(np.uint8).reshape(-1, 2)
        b[:, 4:8] = ((ls[:, 0::2] & 15) | ((ls[:, 1::2] & 15) << 4)).astype(np.uint8)
    return out


# ---------------------------------------------------------------------------------------------------------------- fixtures
# gq_dequantize_blocks: IQ4_XS [5, 512] is 10 blocks, one partial turn of 16; [33, 768] is 99, full turns and a partial last;
# IQ4_NL [5, 96]: 15 blocks, a turn straddles rows and C % 256 != 0; [67, 288]: 603 blocks, four full turns of 128 and a rest.
DEQUANT_CASES = [(XS, 5, 512), (XS, 33, 768), (NL, 5, 96), (NL, 67, 288)]
# the packed forward: R = 20 is a 16-row group and a partial one, R = 130 a 128-row tile and two rows
GEMM_CASES = [(XS, 20, 512), (NL, 20, 512), (XS, 130, 512), (NL, 130, 512)]
EXPERT_CASES = [(XS, 3 * 20, 256), (NL, 3 * 20, 256)]   # E = 3 stacked experts of [20, 256]


def dequant_fixture(t, R, C):
    return blocks_with_d(t, R, C, seed=100 + t + R + C)


def gemm_fixture(t, R, C):
    return blocks_with_d(t, R, C, seed=200 + t + R + C, d_bits=gemm_d_bits)


def scales_and_codes(t, blocks):
    """(the set of ls values, the set of 4-bit codes) that occur in the blocks (IQ4_NL has no ls: an empty set)."""
    bs, ts = GEOMETRY[t]
    b = np.ascontiguousarray(blocks, np.uint8).reshape(-1, ts)
    qs = b[:, 2:] if t == NL else b[:, 8:]
    codes = set(np.unique(qs & 15).tolist()) | set(np.unique(qs >> 4).tolist())
    ls = {xs_scale(bytes(row[:8]) + bytes(128), ib) for row in b for ib in range(8)} if t == XS else set()
    return ls, codes
