"""The contract of gq_sample_logits (include/gptq_gguf_sample.h) in numpy fp64: a plain helper of the sampler tests, no test.

    order(z)                               the ranking: lexsort((index, -z)), -0 == +0
    table(z, top_k, top_p, t)              -> dict(ids, w, cdf, n, K): candidates in rank order, their weights, the prefix sums
    sample(z, u, top_k, top_p, t)          -> the token id, or -1

z is one row as float32 (the exact values of the logits)."""
import numpy as np


def order(z):
    z = np.asarray(z, dtype=np.float64) + 0.0  # (-0.0 + 0.0 = +0.0: equal numbers must not be told apart)
    return np.lexsort((np.arange(z.size), -z))


def bad_row(z):
    z = np.asarray(z, dtype=np.float64)
    return bool(np.isnan(z).any() or not np.isfinite(z.max()))


def table(z, top_k, top_p, temperature):
    z = np.asarray(z, dtype=np.float64)
    K = min(int(top_k), z.size)
    ids = order(z)[:K]
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.exp((z[ids] - z[ids[0]]) / float(temperature))
    cdf = np.cumsum(w)
    n = K if top_p == 1 else int(np.argmax(cdf >= float(top_p) * cdf[-1])) + 1
    return dict(ids=ids, w=w, cdf=cdf, n=n, K=K)


def sample(z, u, top_k, top_p, temperature):
    if bad_row(z):
        return -1
    if temperature == 0:
        return int(order(z)[0])
    t = table(z, top_k, top_p, temperature)
    n, cdf = t["n"], t["cdf"]
    hit = np.nonzero(cdf[:n] > float(u) * cdf[n - 1])[0]
    j = int(hit[0]) if hit.size else int(np.nonzero(t["w"][:n] > 0)[0][-1])
    return int(t["ids"][j])
