"""The contract of gq_fwd_moe_combine (include/gptq_gguf_moe_calib.h) restated as plain loops over tokens and pairs, and
transformers' own sequence of launches for comparison.  Test scaffolding only.

Pairs are numbered p = k * T + t (the router's [T, K] index transposed, then flattened)."""
import torch


def route(pair_expert, E):
    """gq_moe_route's rule on a list of ids: expert e's run holds the pairs that name e, ascending; the runs follow each other
    in expert order; an id outside [0, E) is in no run; -1 from the end of the last run on.  -> (expert_start, order)."""
    runs = [[p for p, e in enumerate(pair_expert) if e == x] for x in range(E)]
    start = [0]
    for r in runs:
        start.append(start[-1] + len(r))
    order = [p for r in runs for p in r]
    return start, order + [-1] * (len(pair_expert) - len(order))


def transposed_pairs(top_k_index):
    """[T, K] index -> the list of ids in pair order p = k T + t."""
    return top_k_index.t().reshape(-1).tolist()


def combine_spec(y, top_k_index, w, E):
    """y [P, H] (fp16 / bf16) in expert-sorted order (row s belongs to pair order[s] of route(transposed_pairs(index), E)),
    top_k_index [T, K] integers, w [T, K] fp32 or y's dtype -> out [T, H] of y's dtype, by the header's contract:
    acc = +0; for the token's valid pairs in ascending expert id, ties by k: v = round(float(y[s]) float(w[t, k])),
    acc = round(float(acc) + float(v)).  All on the CPU."""
    y, w = y.cpu(), w.cpu()
    T, K = top_k_index.shape
    dt = y.dtype
    pairs = transposed_pairs(top_k_index.cpu())
    _, order = route(pairs, E)
    row_of = {p: s for s, p in enumerate(order) if p >= 0}
    out = torch.zeros(T, y.shape[1], dtype=dt)
    for t in range(T):
        entries = sorted((pairs[k * T + t], k) for k in range(K) if 0 <= pairs[k * T + t] < E)
        acc = torch.zeros(y.shape[1], dtype=dt)  # +0
        for _, k in entries:
            v = (y[row_of[k * T + t]].float() * w[t, k].float()).to(dt)
            acc = (acc.float() + v.float()).to(dt)
        out[t] = acc
    return out


def combine_hf(y, top_k_index, w, E):
    """What transformers' MixtralExperts.forward does with the experts' outputs, on y's device: per hit expert in ascending id,
    h = y_e * w[token_idx, top_k_pos, None]; final.index_add_(0, token_idx, h.to(final.dtype)).  y in expert-sorted order."""
    T, K = top_k_index.shape
    final = torch.zeros(T, y.shape[1], dtype=y.dtype, device=y.device)
    at = 0
    for e in range(E):
        top_k_pos, token_idx = torch.where((top_k_index == e).T)
        n = token_idx.numel()
        if n == 0:
            continue
        h = y[at:at + n] * w[token_idx, top_k_pos, None]
        final.index_add_(0, token_idx, h.to(final.dtype))
        at += n
    return final


def bits(t):
    return t.contiguous().view(torch.int16)
