"""Fitness / quality metrics of a (quantized) causal LM on token-id sequences: perplexity, dense KL and top-k sparse KL
against a target model's logits -- the interface of the reference's evopress/src/metrics.py:10-119 (and of
quant/gptq/src/metrics.py:7-33, which is its first function), on the gq_eval_* kernels.

What differs from the reference, on purpose:
  * the next-token shift is made with labels (the last position of every sequence gets IGNORE) or with row views; the
    `[:, :-1, :].contiguous()` copy of the logits is never made, and there is no 1024-row chunking and no empty_cache():
    the kernels keep no intermediates;
  * every reference running mean is weighted by element counts, i.e. it IS the plain mean over all scored rows.  That mean
    is computed directly: per-row fp32 values summed in fp64 on the device, one host read at the end of a call.  The
    reference's running value carries the logits dtype, so with fp16 logits it is rounded to fp16 after every batch; ours
    is not (with fp32 logits the two agree to fp32 rounding).
`data`: a list of [1, L] id tensors (sequences of one batch must have one length, as in the reference's torch.cat)."""
import math
import os
import random

import numpy as np
import torch

from . import ops

IGNORE = -100


def fix_seed(seed: int):
    """common_utils.py:10-14 of the reference."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.backends.cudnn.deterministic = True


def load_eval_data(path_or_name, num_tokens, seq_len, what="eval_datasets"):
    """Evaluation ids from the reference's `.pt` branch (data_utils.py:134-136, as quant.load_calibration): a list of
    [1, L] id tensors, at most num_tokens // seq_len of them (all when num_tokens is None), cut to seq_len."""
    if os.path.isfile(path_or_name):
        data = torch.load(path_or_name)
        if num_tokens is not None:
            data = data[: num_tokens // seq_len]
        return [s[:, :seq_len] for s in data]
    raise ValueError(f"{what} must be a .pt file of token-id tensors (got {path_or_name!r}); "
                     "dataset downloads are not part of this package")


def _device(model):
    return next(model.parameters()).device


def _batch(items, i, j, device):
    return (items[i] if j - i == 1 else torch.cat(items[i:j])).to(device)


@torch.no_grad()
def nll_rows(model, data, batch_size: int = 1) -> torch.Tensor:
    """fp32 [sum of B * (L - 1)]: the negative log-likelihood of every scored position, in order (on the model's device)."""
    device = _device(model)
    out = []
    for i in range(0, len(data), batch_size):
        j = min(i + batch_size, len(data))
        inputs = _batch(data, i, j, device)
        logits = model(inputs).logits  # [B, L, V]: all B * L rows go to the kernel, the last of a sequence is ignored
        labels = torch.full_like(inputs, IGNORE)
        labels[:, :-1] = inputs[:, 1:]
        out.append(ops.eval_nll(logits, labels, IGNORE)[:, :-1].reshape(-1))
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.float32, device=device)


@torch.no_grad()
def compute_perplexity(model, data, batch_size: int = 1, logits_fn=None) -> float:
    """exp(mean NLL of the next token) over all sequences (metrics.py:10-37).  logits_fn(i, inputs) -> [1, L, V], when given,
    stands for model(inputs).logits of sequence i (suffix_forward: a forward from a cached block boundary)."""
    assert logits_fn is None or batch_size == 1
    device = _device(model)
    total, rows = torch.zeros((), dtype=torch.float64, device=device), 0
    for i in range(0, len(data), batch_size):
        j = min(i + batch_size, len(data))
        inputs = _batch(data, i, j, device)
        logits = model(inputs).logits if logits_fn is None else logits_fn(i, inputs)
        labels = torch.full_like(inputs, IGNORE)
        labels[:, :-1] = inputs[:, 1:]
        total += ops.eval_nll(logits, labels, IGNORE).sum(dtype=torch.float64)  # ignored rows are exact zeros
        rows += inputs.shape[0] * (inputs.shape[1] - 1)
    return math.exp(total.item() / rows)


@torch.no_grad()
def compute_kl_div(model, data, target_logits, batch_size: int = 1, logits_fn=None) -> float:
    """mean over rows of KL(softmax(target) || softmax(model)), the last position of a sequence left out
    (metrics.py:41-86).  target_logits: a list of [1, L, V] tensors (collect_target_logits).  logits_fn: as
    compute_perplexity's."""
    assert logits_fn is None or batch_size == 1
    device = _device(model)
    total, rows = torch.zeros((), dtype=torch.float64, device=device), 0
    for i in range(0, len(data), batch_size):
        j = min(i + batch_size, len(data))
        inputs = _batch(data, i, j, device)
        targets = _batch(target_logits, i, j, device)
        logits = model(inputs).logits if logits_fn is None else logits_fn(i, inputs)
        kl = ops.eval_kl(logits[:, :-1, :], targets[:, :-1, :])  # row views, read in place
        total += kl.sum(dtype=torch.float64)
        rows += kl.numel()
    return total.item() / rows


@torch.no_grad()
def compute_sparse_kl_div(model, data, target_logits, logits_fn=None) -> float:
    """The same over the target's top-k columns only, both softmaxes over those k (metrics.py:89-119).
    target_logits: a list of (topk_values [1, L, k], topk_indices [1, L, k]) pairs.  logits_fn: as compute_perplexity's."""
    device = _device(model)
    total, rows = torch.zeros((), dtype=torch.float64, device=device), 0
    for i in range(len(data)):
        inputs = data[i].to(device)
        vals, ids = (t.to(device) for t in target_logits[i])
        logits = model(inputs).logits if logits_fn is None else logits_fn(i, inputs)
        kl = ops.eval_kl_sparse(logits[:, :-1, :], vals[:, :-1, :], ids[:, :-1, :])
        total += kl.sum(dtype=torch.float64)
        rows += kl.numel()
    return total.item() / rows


@torch.no_grad()
def collect_target_logits(model, data, topk=None):
    """The target side of the two KL metrics (evo_quant_search.py:361-373): per sequence the model's logits [1, L, V], or
    with topk the pair (topk_values, topk_indices) of logits.topk(topk, dim=-1).  Kept on the model's device and in its
    dtype (the reference moves them to the host)."""
    device = _device(model)
    out = []
    for ids in data:
        logits = model(ids.to(device)).logits
        if topk is None:
            out.append(logits)
        else:
            v, idx = logits.topk(k=topk, dim=-1)
            out.append((v, idx))
    return out
