"""Inputs the Q8_0 tests share (tests/test_q8_cpu.py pins them on the host, tests/test_gpu_q8.py runs them on the GPU)."""
import numpy as np


def crafted_encoder_matrix() -> np.ndarray:
    """float32 [4, 32], one block per row:
      0  exact halves with d = 1 (amax 127): roundf rounds them AWAY from zero, round-to-even would not;
      1  all zero but one -0.0: d = 0, id = 0, every code 0;
      2  ~1e7: d = amax / 127 ~ 78740 overflows fp16 (stored inf) while the codes come from the fp32 d;
      3  ~1e-4: d ~ 7.9e-7 is an fp16 subnormal."""
    rng = np.random.default_rng(7)
    x = np.zeros((4, 32), np.float32)
    x[0, :9] = [127, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, -126.5]
    x[1, 5] = -0.0
    x[2] = rng.uniform(-1, 1, 32).astype(np.float32) * np.float32(1e7)
    x[2, 3] = 1e7
    x[3] = rng.uniform(-1, 1, 32).astype(np.float32) * np.float32(1e-4)
    x[3, 11] = -1e-4
    return x


HALVES_AWAY = [127, 1, 2, 3, -1, -2, -3, 127, -127]   # what row 0 must encode to
HALVES_EVEN = [127, 0, 2, 2, 0, -2, -2, 126, -126]    # what round-half-to-even would give


def random_encoder_matrix() -> np.ndarray:
    """float32 [2048, 1024]: 65536 blocks of standard normal values.  Among them are a few codes where round(x / d) and
    round(x * (1 / d)) differ (division_and_reciprocal_differ finds them): the product with the reciprocal is the contract."""
    return np.random.default_rng(0).standard_normal((1 << 16, 32), dtype=np.float32).reshape(2048, 1024)


def division_and_reciprocal_differ(x: np.ndarray) -> np.ndarray:
    """Block indices of x (viewed [-1, 32]) where a code computed as roundf(x / d) is not the contract's roundf(x * id)."""
    b = np.ascontiguousarray(x, np.float32).reshape(-1, 32)
    d = np.abs(b).max(axis=1, keepdims=True) / np.float32(127)
    safe = np.where(d == 0, np.float32(1), d)
    rnd = lambda v: np.sign(v) * np.floor(np.abs(v) + 0.5)  # noqa: E731  (roundf of an fp32 value, in exact fp64 arithmetic)
    by_div = rnd((b / safe).astype(np.float64))                     # the fp32 quotient
    by_mul = rnd((b * (np.float32(1) / safe)).astype(np.float64))   # the fp32 product with the fp32 reciprocal
    return np.nonzero((by_div != by_mul).any(axis=1))[0]
