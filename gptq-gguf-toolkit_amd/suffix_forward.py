"""Evaluate a search candidate from its first changed block on, and split a selection's candidates over the ranks.

A candidate of evo_quant_search differs from its parent in a few Linears.  Every block before the first changed one sees the
parent's weights and the parent's inputs, so its output is the parent's: the parent is run ONCE over the minibatch
(`SuffixRunner.capture`), the hidden states at block boundaries are kept, and a candidate runs only the blocks from the
nearest kept boundary at or before its first changed block (`SuffixRunner.logits`).  The same fitness is the same number
whichever rank computes it, so a selection's candidates are also dealt to the ranks (`assign_candidates`) and the fitnesses
all-gathered as fp64 (`Ranks`).  The contract of both: for a seed the search's trajectory -- trace, configuration, every
fitness up to the repeatability of the forward itself -- is the one of the plain loop.

The pure parts (no torch): first_changed_block, cached_boundaries, cache_bytes, choose_stride, plan_stage, stage_costs,
assign_candidates.  Under ranks the candidate-to-rank map comes from stage_costs alone; the stride and whether to reuse are each
rank's own decision for its own share (its free memory is nobody else's), made after the map is fixed.

Memory: boundaries x tokens x hidden x element_size bytes, where the boundaries are the inputs of blocks 0, s, 2s, ... and the
input of the post-block modules (the parent itself, competing in the last stage, then costs no block at all).  At stride 1
that is (n_blocks + 1) x 16384 x 4096 x 2 = 4.4 GB for Llama-3-8B at 16384 tokens and 21.7 GB for 70B.  choose_stride takes
the smallest s whose cache fits the budget, or None (no reuse for that stage)."""
import weakref
from typing import Callable, Dict, List, Optional, Sequence, Tuple

from .model_utils import ForwardInterrupt


# ------------------------------------------------------------------------------------------------ pure functions
def block_of(layer_name: str) -> int:
    """The block index of a Linear's name, by the rule of evo_quant_search.layer_order_fn: `model.layers.<b>.…`."""
    return int(layer_name.split(".")[2])


def first_changed_block(parent_flat: Dict[str, float], cand_flat: Dict[str, float], n_blocks: int) -> int:
    """The smallest block index among the Linears whose level differs; n_blocks when none does (only the post-block
    modules then run: the parent competing in the last stage)."""
    changed = [block_of(n) for n, bw in cand_flat.items() if parent_flat[n] != bw]
    return min(changed) if changed else n_blocks


def cached_boundaries(n_blocks: int, stride: int) -> List[int]:
    """Boundary b is the hidden-state input of block b; boundary n_blocks the input of the post-block modules.  Kept: every
    stride-th one from 0, and the last."""
    assert n_blocks >= 1 and stride >= 1
    return list(range(0, n_blocks, stride)) + [n_blocks]


def cache_bytes(n_blocks: int, stride: int, tokens: int, hidden: int, element_size: int) -> int:
    return len(cached_boundaries(n_blocks, stride)) * tokens * hidden * element_size


def choose_stride(n_blocks: int, tokens: int, hidden: int, element_size: int, budget_bytes: int) -> Optional[int]:
    """The smallest stride whose cache fits budget_bytes; None when even stride n_blocks (boundary 0 and the last) does not."""
    for s in range(1, n_blocks + 1):
        if cache_bytes(n_blocks, s, tokens, hidden, element_size) <= budget_bytes:
            return s
    return None


def start_boundary(first_changed: int, n_blocks: int, stride: int) -> int:
    """The nearest kept boundary at or before `first_changed`."""
    return n_blocks if first_changed >= n_blocks else (first_changed // stride) * stride


def plan_stage(cands_flat: Sequence[Dict[str, float]], parent_flat: Dict[str, float], n_blocks: int,
               stride: Optional[int]) -> Tuple[bool, List[int]]:
    """-> (reuse?, each candidate's start boundary, in candidate order) for the candidates ONE process evaluates (under ranks:
    this rank's share -- every rank plans for itself, with its own stride).  A candidate started at boundary b runs
    n_blocks - b blocks instead of n_blocks; filling the cache costs this process n_blocks block forwards.  Reuse only when
    the block forwards saved exceed those of the capture.  A parent that is itself among these candidates starts at
    n_blocks: its evaluation IS the capture, so the two cancel.  stride None (the cache does not fit): no reuse.  All starts
    are 0 when the stage does not reuse.  Pure: no rng, the order is the candidates'."""
    if stride is None or not cands_flat:
        return False, [0] * len(cands_flat)
    starts = [start_boundary(first_changed_block(parent_flat, c, n_blocks), n_blocks, stride) for c in cands_flat]
    if sum(starts) > n_blocks:
        return True, starts
    return False, [0] * len(cands_flat)


def stage_costs(cands_flat: Sequence[Dict[str, float]], parent_flat: Dict[str, float], n_blocks: int) -> List[float]:
    """What assign_candidates balances when a stage may reuse: the blocks a candidate runs from its first changed block.
    A function of the candidates and the parent ALONE -- not of a stride, a budget or whether any rank ends up reusing,
    which each rank decides for itself from its own free memory -- so every rank computes the same assignment."""
    return [float(n_blocks - first_changed_block(parent_flat, c, n_blocks)) for c in cands_flat]


def assign_candidates(costs: Sequence[float], world_size: int) -> List[int]:
    """The rank of every candidate: longest cost first, each to the least loaded rank, ties by candidate index and then by
    rank (dist_utils.assign_owners' rule).  The loads differ by at most one candidate's cost; equal costs deal candidate i to
    rank i % world_size.  Deterministic; the same on every rank as long as `costs` is (stage_costs is, a stride is not)."""
    loads, owner = [0.0] * world_size, [0] * len(costs)
    for i in sorted(range(len(costs)), key=lambda k: (-costs[k], k)):
        r = min(range(world_size), key=lambda k: (loads[k], k))
        owner[i] = r
        loads[r] += costs[i]
    return owner


# ------------------------------------------------------------------------------------------------ the ranks
class Ranks:
    """The process group as selection() needs it: who am I, and ONE collective -- every rank's fitnesses to every rank."""

    def __init__(self, device="cpu"):
        import torch.distributed as dist
        self.rank, self.world_size, self.device = dist.get_rank(), dist.get_world_size(), device

    def gather(self, mine: Sequence[float]):
        """mine: this rank's fp64 vector (one entry per candidate, whatever it did not evaluate is ignored)
        -> [world_size][len(mine)] nested lists of Python floats, the same on every rank."""
        import torch
        import torch.distributed as dist
        v = torch.tensor(list(mine), dtype=torch.float64, device=self.device)
        out = torch.empty(self.world_size * v.numel(), dtype=torch.float64, device=self.device)
        dist.all_gather_into_tensor(out, v)
        return out.view(self.world_size, v.numel()).tolist()


# ------------------------------------------------------------------------------------------------ the runner
_USE_CACHE_CHECKED = weakref.WeakSet()  # the models whose use_cache=False forward has been compared with the plain call


class _Seq:
    __slots__ = ("shape", "hidden", "args", "kwargs")


def _first(x):
    return x[0] if isinstance(x, (tuple, list)) else x  # a block returns a tensor or a tuple (quantizer._first)


class SuffixRunner:
    """capture(data) / logits(i, start_block) / invalidate() around a causal LM whose decoder blocks are
    model.get_submodule(blocks) and whose logits are post_blocks applied in turn to the last block's output."""

    def __init__(self, model, blocks: str = "model.layers", post_blocks: Sequence[str] = ("model.norm", "lm_head"),
                 budget_bytes: Optional[int] = None, log: Callable = print):
        self.model, self.blocks = model, model.get_submodule(blocks)
        self.post = [model.get_submodule(n) for n in post_blocks]
        self.n_blocks, self.budget_bytes, self.log = len(self.blocks), budget_bytes, log
        self.stride: Optional[int] = None
        self.strides_used: List[Optional[int]] = []  # one entry per stride_for call (observable)
        self.captures = 0
        self._seqs: List[_Seq] = []

    # ---- memory ----
    def _param(self):
        return next(self.model.parameters())

    def stride_for(self, data) -> Optional[int]:
        """The stride this minibatch's cache is kept at (choose_stride), None when it does not fit.  The budget is
        budget_bytes, else the device memory that is free now (the allocator's unused reserve included) less what one
        forward takes: a reserve of 1 GiB plus four logits tensors of the longest sequence.  Besides the hidden states the
        cache holds, once per sequence, what the blocks receive: with eager attention that is an L x L mask in the model
        dtype (134 MB for 8192 tokens in 16 bits), taken off the free memory here (an explicit budget_bytes is for the
        hidden states alone); position ids and embeddings (a few L x
        head_dim) are not counted.  The answer depends on THIS process's free memory: ranks may differ, and nothing that
        must be the same on every rank is derived from it."""
        import torch
        p = self._param()
        tokens = sum(int(ids.shape[0] * ids.shape[1]) for ids in data)
        budget = self.budget_bytes
        if budget is None:
            if p.device.type != "cuda":
                budget = 1 << 62
            else:
                free = torch.cuda.mem_get_info(p.device)[0] + torch.cuda.memory_reserved(p.device) - \
                    torch.cuda.memory_allocated(p.device)
                longest = max(int(ids.shape[0] * ids.shape[1]) for ids in data)
                budget = free - (1 << 30) - 4 * longest * self.model.config.vocab_size * p.element_size()
                if getattr(self.model.config, "_attn_implementation", None) == "eager":
                    budget -= self.mask_bytes(data)
        s = choose_stride(self.n_blocks, tokens, self.model.config.hidden_size, p.element_size(), budget)
        self.strides_used.append(s)
        if s is None:
            self.log(f"reuse_prefix: the hidden states of {tokens} tokens at 2 boundaries need "
                     f"{cache_bytes(self.n_blocks, self.n_blocks, tokens, self.model.config.hidden_size, p.element_size())} "
                     f"bytes, {max(budget, 0)} are available: this stage runs every candidate in full")
        return s

    def mask_bytes(self, data) -> int:
        """The [1, 1, L, L] causal masks eager attention is handed, one per sequence, in the model dtype."""
        return sum(int(ids.shape[0]) * int(ids.shape[1]) ** 2 for ids in data) * self._param().element_size()

    # ---- capture ----
    def _check_use_cache(self, inputs) -> None:
        """Once per model: the forward under use_cache=False gives the logits of metrics' own call model(inputs).  Where
        two such calls differ from each other (a forward that does not repeat), their spread is the bound."""
        a, b = self.model(inputs).logits.float(), self.model(inputs).logits.float()
        c = self.model(inputs, use_cache=False).logits.float()
        spread, diff = float((a - b).abs().max()), float((a - c).abs().max())
        assert diff <= spread, (f"model(inputs, use_cache=False) differs from model(inputs) by {diff!r} (two plain calls "
                                f"differ by {spread!r}): the prefix cannot be reused on this model")
        _USE_CACHE_CHECKED.add(self.model)

    def capture(self, data, stride: Optional[int] = None) -> None:
        """Run the CURRENT weights (the parent's) over every sequence of `data` -- one [1, L] sequence per call, as metrics
        batches them -- up to the post-block modules, keeping the hidden-state input of the kept boundaries and, once per
        sequence, what the blocks receive besides it (position embeddings, mask, position ids: independent of the weights)."""
        import torch
        self.invalidate()
        if stride is None:
            stride = self.stride_for(data)
            if stride is None:
                raise MemoryError("reuse_prefix: the cache does not fit (ask stride_for first)")
        device = self._param().device
        keep = cached_boundaries(self.n_blocks, stride)
        with torch.no_grad():
            for ids in data:
                inputs = ids.to(device)
                if self.model not in _USE_CACHE_CHECKED:
                    self._check_use_cache(inputs)
                seq = _Seq()
                seq.shape, seq.hidden, seq.args, seq.kwargs = tuple(inputs.shape), {}, None, None

                def see_block(b, module, args, kwargs, seq=seq):
                    seq.hidden[b] = (args[0] if len(args) > 0 else kwargs["hidden_states"]).detach().clone()
                    if seq.args is None:
                        seq.args = tuple(args[1:])
                        seq.kwargs = {k: v for k, v in kwargs.items() if k != "hidden_states" or len(args) > 0}
                        # no per-call state: a KV cache among the arguments would be appended to by every replay
                        held = [k for k in ("past_key_values", "past_key_value") if seq.kwargs.get(k) is not None]
                        assert not held, f"the blocks received a cache object ({held}) under use_cache=False"

                def see_post(module, args, seq=seq):
                    seq.hidden[self.n_blocks] = args[0].detach().clone()
                    raise ForwardInterrupt  # the logits of the capture are nobody's: lm_head is not run

                hooks = [self.blocks[b].register_forward_pre_hook(
                    (lambda m, a, kw, b=b: see_block(b, m, a, kw)), with_kwargs=True) for b in keep[:-1]]
                hooks.append(self.post[0].register_forward_pre_hook(see_post))
                try:
                    self.model(inputs, use_cache=False)
                    raise RuntimeError("the post-block modules were never reached")
                except ForwardInterrupt:
                    pass
                finally:
                    for h in hooks:
                        h.remove()
                assert sorted(seq.hidden) == keep, (sorted(seq.hidden), keep)
                self._seqs.append(seq)
        self.stride = stride
        self.captures += 1

    def invalidate(self) -> None:
        self._seqs, self.stride = [], None

    @property
    def valid(self) -> bool:
        return self.stride is not None

    # ---- replay ----
    def logits(self, i: int, start_block: int, inputs=None):
        """The logits of sequence i of the captured minibatch under the CURRENT weights, which must equal the captured ones
        in every block before start_block: the blocks from the nearest kept boundary at or before start_block, then the
        post-block modules.  `inputs`, when given, must have the captured sequence's shape."""
        import torch
        assert self.valid, "no captured minibatch (capture() first; the cache is dropped at the end of every stage)"
        assert 0 <= start_block <= self.n_blocks
        seq = self._seqs[i]
        assert inputs is None or tuple(inputs.shape) == seq.shape, (tuple(inputs.shape), seq.shape)
        b = max(k for k in seq.hidden if k <= start_block)
        h = seq.hidden[b]
        with torch.no_grad():
            for k in range(b, self.n_blocks):
                h = _first(self.blocks[k](h, *seq.args, **seq.kwargs))
            for m in self.post:
                h = m(h)
        return h


class StageReuse:
    """What selection() is handed: the plan of a stage and the capture behind it.  store: flatten(state) and switch(state)
    (level_store.LevelStore); runner: n_blocks, stride_for(data), capture(data, stride), invalidate() (SuffixRunner)."""

    def __init__(self, runner, store):
        self.runner, self.store = runner, store
        self.stages = []  # (reuse?, stride, starts) per stage (observable)

    def costs(self, candidates, parent) -> List[float]:
        """stage_costs of the stage's candidates: the same list on every rank."""
        flat = self.store.flatten
        return stage_costs([flat(c) for c in candidates], flat(parent), self.runner.n_blocks)

    def begin_stage(self, candidates, parent, data) -> Optional[List[int]]:
        """candidates: those THIS process evaluates -> their start boundaries, or None when it does not reuse in this
        stage (its own decision: own stride, own share).  Captures nothing yet."""
        self.runner.invalidate()
        if parent is None or not candidates:
            return None
        stride = self.runner.stride_for(data)
        flat = self.store.flatten
        reuse, starts = plan_stage([flat(c) for c in candidates], flat(parent), self.runner.n_blocks, stride)
        self.stages.append((reuse, stride, starts))
        self._stride = stride
        return starts if reuse else None

    def capture(self, parent, data) -> None:
        """Make the parent current and fill the cache."""
        self.store.switch(parent)
        self.runner.capture(data, self._stride)

    def end_stage(self) -> None:
        self.runner.invalidate()
