"""Prefix reuse and ranks of the bit-width search, host side (no GPU): suffix_forward's pure functions (first changed block,
cache arithmetic, stage plan, rank assignment), SuffixRunner on a 4-block Llama in fp32 on the CPU, and search() with a fake
fitness -- alone, with a stage plan, under two gloo ranks -- against the plain loop's trace and the reference's trajectory
(fixture G19)."""
import os
import random
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from test_search_cpu import CALIB, fake_fitness, problem

torch = pytest.importorskip("torch")
mp = torch.multiprocessing

KINDS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
         "mlp.down_proj")


def flat(n_blocks, changes=(), base=4.0):
    """{name: level} of an n_blocks model, every Linear at `base` except `changes` = ((block, kind, level), ...)."""
    out = {f"model.layers.{b}.{k}": base for b in range(n_blocks) for k in KINDS}
    for b, k, lv in changes:
        out[f"model.layers.{b}.{k}"] = lv
    return out


# ------------------------------------------------------------------------------------------------ pure functions
def test_first_changed_block():
    from gptq_gguf_toolkit_amd import suffix_forward as F
    from gptq_gguf_toolkit_amd.evo_quant_search import layer_order_fn
    par = flat(12)
    assert all(F.block_of(n) == layer_order_fn(n)[0] for n in par)  # one rule: block 10 is no "1"
    assert F.first_changed_block(par, flat(12), 12) == 12           # the parent itself: only the post-block modules run
    assert F.first_changed_block(par, flat(12, [(11, "mlp.down_proj", 2.0)]), 12) == 11
    assert F.first_changed_block(par, flat(12, [(0, "self_attn.q_proj", 6.0)]), 12) == 0
    assert F.first_changed_block(par, flat(12, [(10, "mlp.up_proj", 2.0), (2, "mlp.up_proj", 6.0), (7, "mlp.up_proj", 6.0)]), 12) == 2
    # dict order plays no part
    cand = dict(reversed(list(flat(12, [(5, "self_attn.v_proj", 2.0), (9, "self_attn.v_proj", 6.0)]).items())))
    assert F.first_changed_block(par, cand, 12) == 5


def test_cache_arithmetic_and_stride():
    from gptq_gguf_toolkit_amd import suffix_forward as F
    assert F.cached_boundaries(4, 1) == [0, 1, 2, 3, 4] and F.cached_boundaries(4, 2) == [0, 2, 4]
    assert F.cached_boundaries(4, 3) == [0, 3, 4] and F.cached_boundaries(4, 4) == [0, 4] and F.cached_boundaries(5, 2) == [0, 2, 4, 5]
    # Llama-3-8B and 70B at 16384 tokens in 16 bits: the block inputs are 4.3 GB and 21.5 GB, the post-block input one more
    assert F.cache_bytes(32, 1, 16384, 4096, 2) == 33 * 16384 * 4096 * 2 == 4429185024
    assert F.cache_bytes(80, 1, 16384, 8192, 2) == 81 * 16384 * 8192 * 2
    one = 16384 * 4096 * 2
    assert F.choose_stride(32, 16384, 4096, 2, 33 * one) == 1 and F.choose_stride(32, 16384, 4096, 2, 33 * one - 1) == 2
    assert F.choose_stride(32, 16384, 4096, 2, 17 * one) == 2 and F.choose_stride(32, 16384, 4096, 2, 12 * one) == 3
    assert F.choose_stride(32, 16384, 4096, 2, 3 * one) == 16 and F.choose_stride(32, 16384, 4096, 2, 2 * one) == 32  # [0, 32]
    assert F.choose_stride(32, 16384, 4096, 2, 2 * one - 1) is None and F.choose_stride(32, 16384, 4096, 2, 0) is None
    for s in (1, 2, 3, 4):
        for fc in range(5):
            b = F.start_boundary(fc, 4, s)
            assert b in F.cached_boundaries(4, s) and b <= fc and not any(b < k <= fc for k in F.cached_boundaries(4, s))


def test_stage_plan():
    from gptq_gguf_toolkit_amd import suffix_forward as F
    n = 8
    par = flat(n)
    last = flat(n, [(7, "mlp.down_proj", 2.0), (7, "mlp.up_proj", 6.0)])
    mid = flat(n, [(5, "self_attn.q_proj", 2.0), (6, "self_attn.q_proj", 6.0)])
    first = flat(n, [(0, "mlp.up_proj", 2.0), (7, "mlp.up_proj", 6.0)])
    cands = [mid, first, last, par]
    # stride 1: every first changed block is a boundary; the parent among the candidates starts at n (no block at all)
    assert F.plan_stage(cands, par, n, 1) == (True, [5, 0, 7, 8])
    # stride 2 and 3: the nearest kept boundary at or before; stride n: boundary 0 and the last only
    assert F.plan_stage(cands, par, n, 2) == (True, [4, 0, 6, 8])
    assert F.plan_stage(cands, par, n, 3) == (True, [3, 0, 6, 8])
    assert F.plan_stage(cands, par, n, n) == (False, [0, 0, 0, 0])   # saves the parent's 8 only: the capture's own cost
    # declined: nothing saved (block 0), no more saved than the capture costs, the cache does not fit
    assert F.plan_stage([first, first], par, n, 1) == (False, [0, 0])
    assert F.plan_stage([mid], par, n, 1) == (False, [0]) and F.plan_stage([last], par, n, 1) == (False, [0])
    assert F.plan_stage([mid, flat(n, [(3, "mlp.up_proj", 2.0)])], par, n, 1) == (False, [0, 0])       # 5 + 3 = 8, not more
    assert F.plan_stage([mid, flat(n, [(4, "mlp.up_proj", 2.0)])], par, n, 1) == (True, [5, 4])        # 9 > 8
    assert F.plan_stage(cands, par, n, None) == (False, [0, 0, 0, 0]) and F.plan_stage([], par, n, 1) == (False, [])
    # the parent with one more candidate: its own evaluation is the capture, so any saving of the other one decides
    assert F.plan_stage([last, par], par, n, 1) == (True, [7, 8]) and F.plan_stage([first, par], par, n, 1) == (False, [0, 0])
    # what the ranks balance: blocks from the first changed block -- no stride, no budget in it, so every rank's list is the same
    assert F.stage_costs(cands, par, n) == [3.0, 8.0, 1.0, 0.0] and F.stage_costs([], par, n) == []
    # the order is the candidates'
    assert F.plan_stage(cands[::-1], par, n, 1) == (True, [8, 7, 0, 5])


def test_rank_assignment_is_a_balanced_partition():
    from gptq_gguf_toolkit_amd import suffix_forward as F
    rng = random.Random(4)
    for world in (1, 2, 3, 8):
        for n in (0, 1, 5, 8, 32, 33):
            for costs in ([1.0] * n, [float(rng.randint(0, 32)) for _ in range(n)]):
                owner = F.assign_candidates(costs, world)
                assert owner == F.assign_candidates(list(costs), world)  # nothing but the arguments: no rank is asked
                assert len(owner) == n and all(0 <= r < world for r in owner)  # a partition: every candidate one rank
                loads = [sum(c for c, r in zip(costs, owner) if r == k) for k in range(world)]
                assert max(loads) - min(loads) <= (max(costs) if costs else 0)
    assert F.assign_candidates([1.0] * 7, 3) == [0, 1, 2, 0, 1, 2, 0]   # equal costs: ceil(n / world) on the fullest rank
    assert F.assign_candidates([3.0, 8.0, 8.0, 0.0, 5.0], 2) == [1, 0, 1, 1, 0]  # 8 | 8, then 5 to rank 0 (a tie: the lower rank), 3 and 0 to rank 1


# ------------------------------------------------------------------------------------------------ the runner on the CPU
def llama(blocks=4, dtype=torch.float32, seed=0):
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=blocks, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=512, max_position_embeddings=128, rms_norm_eps=1e-5,
                      tie_word_embeddings=False, attn_implementation="eager")
    torch.manual_seed(seed)
    return LlamaForCausalLM(cfg).to(dtype).eval()


def test_runner_on_the_cpu_suffix_equals_full():
    from gptq_gguf_toolkit_amd.suffix_forward import SuffixRunner
    model = llama()
    assert model.config.use_cache  # the plain call makes a KV cache; the capture must not hand one to the replay
    g = torch.Generator().manual_seed(5)
    data = [torch.randint(0, 512, (1, 64), generator=g), torch.randint(0, 512, (1, 37), generator=g)]
    with torch.no_grad():
        want = [model(ids).logits for ids in data]
    ran = []
    hooks = [blk.register_forward_hook(lambda m, a, o, b=b: ran.append(b)) for b, blk in enumerate(model.model.layers)]
    for budget, stride in ((None, 1), (3 * 101 * 256 * 4, 2), (2 * 101 * 256 * 4, 4)):
        runner = SuffixRunner(model, budget_bytes=budget)
        runner.capture(data)
        assert runner.stride == stride and runner.strides_used == [stride] and runner.valid
        for i in range(2):
            for b in range(5):
                del ran[:]
                for _ in range(2):  # twice: a replay leaves the cache as it found it
                    assert torch.equal(runner.logits(i, b, data[i]), want[i]), (stride, i, b)
                first = 4 if b == 4 else (b // stride) * stride
                assert ran == 2 * list(range(first, 4)), (stride, b, ran)
        with pytest.raises(AssertionError):
            runner.logits(0, 1, data[1])  # another sequence's shape
        runner.invalidate()
        with pytest.raises(AssertionError, match="no captured minibatch"):
            runner.logits(0, 0)
    # a changed suffix: blocks 0 and 1 are the captured ones, block 2 on the new ones
    runner = SuffixRunner(model)
    runner.capture(data)
    with torch.no_grad():
        model.model.layers[2].mlp.down_proj.weight.mul_(0.5)
        changed = model(data[1]).logits
    assert not torch.equal(changed, want[1]) and torch.equal(runner.logits(1, 2), changed)
    assert SuffixRunner(model, budget_bytes=1000, log=lambda *a: None).stride_for(data) is None
    for h in hooks:
        h.remove()


# ------------------------------------------------------------------------------------------------ search(): plan and ranks
class FakeRunner:
    def __init__(self, n_blocks, stride=1):
        self.n_blocks, self.stride, self.captured, self.live = n_blocks, stride, 0, False

    def stride_for(self, data):
        return self.stride

    def capture(self, data, stride):
        assert stride == self.stride
        self.captured, self.live = self.captured + 1, True

    def invalidate(self):
        self.live = False


class FakeStore:
    def __init__(self, names):
        self.names, self.switched = names, []

    def flatten(self, state):
        return {n: k for ns, ks in zip(self.names, state) for n, k in zip(ns, ks)}

    def switch(self, state):
        self.switched.append(state)


def planned(ctx, evaluate, log):
    """The fake fitness as main()'s evaluate: it takes a start block, and says what it was asked."""
    def ev(candidate, data, targets, start_block=None):
        log.append(start_block)
        return evaluate(candidate, data, targets)
    return ev


ARGS = dict(generations=5, offspring=8, target_bitwidth=4.0, survivors_per_selection=(3, 1), tokens_per_selection=(100, 200),
            group_rule="size", fitness_fn="ppl")
ARGS2 = dict(ARGS, offspring=16)  # two ranks, two captures: a stage reuses from about 8 candidates on


def test_search_with_a_stage_plan_keeps_the_trace():
    from gptq_gguf_toolkit_amd.suffix_forward import StageReuse
    S, ctx, _ = problem("size", 4.0, blocks=6)
    plain = S.search(ctx, fake_fitness(ctx), CALIB, random.Random(7), **ARGS)
    runner, store, log = FakeRunner(6), FakeStore(ctx.names), []
    reuse = StageReuse(runner, store)
    got = S.search(ctx, planned(ctx, fake_fitness(ctx), log), CALIB, random.Random(7), reuse=reuse, **ARGS)
    assert got == plain
    assert len(reuse.stages) == 10 and not runner.live
    used = [st for st in reuse.stages if st[0]]
    assert used and runner.captured == len(used) and len(store.switched) == len(used)  # the parent made current per capture
    n_full = sum(len(st[2]) for st in reuse.stages if not st[0])
    assert log.count(None) == n_full and len(log) == sum(len(st[2]) for st in reuse.stages)
    assert [s for s in log if s is not None] == [s for st in used for s in st[2]]      # in candidate order
    assert any(st[2][-1] == 6 for st in used)  # the parent in a last stage starts after the last block


def test_reference_trajectory_golden_with_plan_and_ranks(monkeypatch):
    """G19 with the new arguments in use: a stage plan and a one-rank group object."""
    sys.path.insert(0, GOLDEN)
    import make_golden_search as M
    from gptq_gguf_toolkit_amd import evo_quant_search as S
    from gptq_gguf_toolkit_amd.suffix_forward import StageReuse
    plain, seen = S.search, []

    class OneRank:
        rank, world_size = 0, 1

        def gather(self, mine):
            return [list(mine)]

    def search(ctx, evaluate, *a, **kw):
        n_blocks = 1 + max(S.layer_order_fn(n)[0] for g in ctx.names for n in g)
        reuse = StageReuse(FakeRunner(n_blocks), FakeStore(ctx.names))
        seen.append(reuse)
        return plain(ctx, lambda c, d, t, start_block=None: evaluate(c, d, t), *a, reuse=reuse, ranks=OneRank(), **kw)

    monkeypatch.setattr(S, "search", search)
    g = load_golden("G19_search")
    for rule in ("size", "name", "none"):
        got_states, got_text = M.ours(rule)
        assert np.array_equal(np.asarray(got_states, dtype=np.float64), g[f"{rule}_states"])
        assert got_text == bytes(g[f"{rule}_config"]).decode()
    # every generation's two stages were planned; with 3 blocks and a first parent above the budget (`name`: every offspring
    # is lowered all over first) not every run finds a stage worth a capture
    assert len(seen) == 3 and all(len(r.stages) == 2 * M.GENERATIONS for r in seen)
    assert any(st[0] for r in seen for st in r.stages)


def _worker(rank, world, port, strides, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gptq_gguf_toolkit_amd.suffix_forward import Ranks, StageReuse
    S, ctx, _ = problem("size", 4.0, blocks=6)
    log = []
    reuse = StageReuse(FakeRunner(6, strides[rank]), FakeStore(ctx.names)) if strides else None
    out = S.search(ctx, planned(ctx, fake_fitness(ctx), log), CALIB, random.Random(7), reuse=reuse, ranks=Ranks("cpu"), **ARGS2)
    ret[rank] = (out, list(log), reuse.runner.captured if reuse else 0)
    dist.barrier()
    dist.destroy_process_group()


# the stride is a rank's own finding (its free memory): the ranks may disagree on it, one may not fit the cache at all
@pytest.mark.parametrize("strides", [None, (1, 1), (1, 2), (3, None), (None, 1)], ids=str)
def test_two_gloo_ranks_return_the_single_process_trace(strides):
    S, ctx, _ = problem("size", 4.0, blocks=6)
    plain = S.search(ctx, fake_fitness(ctx), CALIB, random.Random(7), **ARGS2)
    total = sum(len(st["candidates"]) for rec in plain[2] for st in rec["stages"])
    ret = mp.Manager().dict()
    port = 25000 + 7 * [None, (1, 1), (1, 2), (3, None), (None, 1)].index(strides) + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, strides, ret), nprocs=2, join=True)
    for r in range(2):
        assert ret[r][0] == plain, f"rank {r}"
    n0, n1 = len(ret[0][1]), len(ret[1][1])
    assert n0 + n1 == total and 0 < n0 < total and 0 < n1 < total  # each evaluated its share only, nothing twice, nothing never
    for r in range(2):
        if strides and strides[r] is not None:
            if strides[r] == 1:  # (at a coarser stride a share of about 8 candidates may never be worth a capture)
                assert ret[r][2] > 0 and any(s is not None for s in ret[r][1])  # this rank captured the parent for itself
            assert (ret[r][2] > 0) == any(s is not None for s in ret[r][1])
            assert all(s is None or s % strides[r] == 0 or s == 6 for s in ret[r][1])
        else:
            assert ret[r][2] == 0 and all(s is None for s in ret[r][1])     # no plan, or no room: its share in full


def test_ranks_that_disagree_on_the_map_are_caught():
    """_evaluate_stage checks after the gather that every candidate was evaluated by its owner and by nobody else."""
    from gptq_gguf_toolkit_amd import evo_quant_search as S

    class Lying:  # a group of two in which the other rank evaluated candidate 0 as well and skipped its own
        rank, world_size = 0, 2

        def gather(self, mine):
            n = len(mine) // 2
            return [list(mine), [1.0] * n + [1.0] + [0.0] * (n - 1)]

    with pytest.raises(AssertionError, match="candidate 0 belongs to rank 0 and was evaluated by ranks \\[0, 1\\]"):
        S._evaluate_stage(lambda c, d, t: 1.0, [[[4.0]], [[2.0]]], None, None, None, None, Lying())


def test_cli_flags_default_to_the_plain_search(tmp_path):
    from gptq_gguf_toolkit_amd import evo_quant_search as S
    ids = tmp_path / "ids.pt"
    torch.save([torch.zeros(1, 8, dtype=torch.long)], ids)
    base = ["--model_name_or_path", "none", "--quant_weights_path", str(tmp_path), "--generations", "1", "--offspring", "2",
            "--target_bitwidth", "4", "--survivors_per_selection", "2", "1", "--tokens_per_selection", "8", "16",
            "--calibration_data", str(ids), "--eval_datasets", str(ids)]
    a = S.parse_args(base)
    assert (a.reuse_prefix, a.reuse_prefix_bytes, a.backend, a.trace_out) == ("off", None, None, None)
    a = S.parse_args(base + ["--reuse_prefix", "on", "--reuse_prefix_bytes", "4096", "--backend", "gloo", "--trace_out", "t.json"])
    assert (a.reuse_prefix, a.reuse_prefix_bytes, a.backend, a.trace_out) == ("on", 4096, "gloo", "t.json")
    with pytest.raises(SystemExit):
        S.parse_args(base + ["--reuse_prefix", "maybe"])
