"""Block bytes of the two types this package reads and does not encode (IQ4_NL, IQ4_XS; include/gptq_gguf_iq4.h), for the rate
scripts: every byte uniform, d = +-2^-12 .. 2^-11, so every decode is finite and no 16-bit subnormal (|w| in 2^-12 .. 7.9)."""
import torch

GEOMETRY = {20: (32, 18), 23: (256, 136)}  # ggml type -> (values, bytes) per block


def iq4_blocks(t, R, C, generator):
    """uint8 [R, C / block * bytes] on the generator's device."""
    bs, ts = GEOMETRY[t]
    dev = generator.device
    b = torch.randint(0, 256, (R * C // bs, ts), device=dev, generator=generator, dtype=torch.uint8)
    b[:, 1] = (b[:, 1] & 0x83) | 0x0C  # fp16 d: sign and the two high mantissa bits kept, exponent field 3
    return b.view(R, C // bs * ts)
