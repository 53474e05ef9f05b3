#!/usr/bin/env python3
"""The per-layer bit-width search: the reference's evopress/evo_quant_search.py with its levels resident on the device.

    python -m gptq_gguf_toolkit_amd.evo_quant_search --model_name_or_path HF_DIR --quant_weights_path DB \
        --calibration_data ids.pt --eval_datasets eval.pt --generations G --offspring N --target_bitwidth B \
        --survivors_per_selection 4 1 --tokens_per_selection 2048 16384 [--group_rule size|name|none] \
        [--fitness_fn kl|ppl|sparse_kl] [--targets_on device|cpu] [--resident dense|packed]

The loop of the reference's main() (:401-779) is restated as functions of their arguments -- scan_available_bitwidths (level_db's),
calculate_total_bits, get_next_bitwidth, initial_parent / initial_candidates, mutate, make_offspring, minibatch, selection,
search -- that draw from ONE random.Random in the reference's call order: random.Random(seed) yields what the reference's
module-level `random` yields after fix_seed(seed), so a seed fixes the same trajectory.  A candidate is evaluated as
LevelStore.switch(candidate) (one gq_level_switch launch over the Linears whose level changed; load_layers :110-138 reads a
dense file per changed Linear) followed by metrics.compute_perplexity / compute_kl_div / compute_sparse_kl_div.

What differs from the reference, on purpose:
  * data are `.pt` files of [1, L] id tensors (as ppleval); anything else is refused before any work;
  * --log_wandb is accepted and refused with a message when wandb is not installed;
  * --targets_on device (default): the KL targets stay on the device in the model dtype when they fit next to the level
    store, else (or with `cpu`) they go to the host as in the reference;
  * level files are recognised by level_db.level_key ("4.pth" and "4-Q4_K.pth" both count; the reference's
    filename.split('-')[0] drops the former with a warning), and the --gguf-layers layout is read too;
  * the reference's progress prints inside the mutation ("Can't decrease bits, continue ...") are not made.
  * --resident packed: no dense live copy of the searched Linears (level_store / packed_linear): the forward reads the
    current level's block bytes, a switch launches nothing.  The KL targets are then collected BEFORE the store is built
    (they need the unmodified dense model, which the store frees).  Fitnesses differ from dense residency by fp32
    summation order only, so a trajectory may differ where two candidates are that close.
  * --reuse_prefix on: the parent is run once per minibatch and a candidate from its first changed block on (suffix_forward);
    under `python -m torch.distributed.run --nproc-per-node N -m gptq_gguf_toolkit_amd.evo_quant_search ...` a selection's
    candidates are dealt to the N ranks and the fitnesses all-gathered.  Both keep the trajectory of a seed; [--backend],
    [--reuse_prefix_bytes], [--trace_out FILE], [--report_out FILE].
  * a model with fused experts (transformers' MixtralExperts: gate_up_proj [E, 2I, H], down_proj [E, H, I]) is searched too: the
    three stacked tensors of an experts module are the units `<module>.gate_proj / .up_proj / .down_proj` (level_store), of
    E * R * C elements each (layer_numel), named in the configuration the way config_converter reads them; [--moe_prefill]
    is packed residency's PackedExperts.prefill.
nn.Linear and expert units only."""
import argparse
import copy
import math
import os
import random
import sys
from collections import defaultdict
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

if __package__ in (None, ""):  # run as a script: make the package importable under its alias
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gptq_gguf_toolkit_amd  # noqa: F401
    __package__ = "gptq_gguf_toolkit_amd"

from .level_db import Levels, expert_unit, filename_of, scan_available_bitwidths  # noqa: E402

State = List[List[float]]


# ------------------------------------------------------------------------------------------------ the layers
def layer_order_fn(layer_name: str):
    """evopress/src/model_utils.py:365-369: (block index, the rest of the name)."""
    split_key = layer_name.split(".")
    return (int(split_key[2]), *split_key[3:])


def layer_numel(model, layer_name: str) -> int:
    """The elements of one searchable layer: a Linear's weight, or the E * R * C of the expert unit
    `<experts module>.{gate,up,down}_proj` (gate and up are E * I * H each, half of gate_up_proj; down is down_proj)."""
    unit = expert_unit(layer_name)
    if unit is None:
        return model.get_submodule(layer_name).weight.numel()
    E, H, I = model.get_submodule(unit[0]).down_proj.shape
    return E * H * I


def group_layers(model, layer_names: Sequence[str], group_rule: str) -> Tuple[List[str], ...]:
    """evopress/src/model_utils.py:371-385: groups in order of first appearance."""
    assert group_rule in ("none", "name", "size")
    if group_rule == "none":
        key = lambda n: 0  # noqa: E731
    elif group_rule == "name":
        key = lambda n: n.split(".")[-1]  # noqa: E731
    else:
        key = lambda n: layer_numel(model, n)  # noqa: E731
    groups = defaultdict(list)
    for n in layer_names:
        groups[key(n)].append(n)
    return tuple(groups.values())


# ------------------------------------------------------------------------------------------------ the budget
def calculate_total_bits(current_bitwidths: State, grouped_layer_names, model):
    """:55-64"""
    total_bits = 0
    for g_id in range(len(grouped_layer_names)):
        for l_id, l_name in enumerate(grouped_layer_names[g_id]):
            total_bits += layer_numel(model, l_name) * current_bitwidths[g_id][l_id]
    return total_bits


def target_bits_of(grouped_layer_names, model, target_bitwidth: float) -> int:
    """:394-399: the per-layer products are truncated before they are added."""
    return sum(int(layer_numel(model, n) * target_bitwidth) for g in grouped_layer_names for n in g)


def get_next_bitwidth(current_bitwidths: State, target_bits, grouped_layer_names, available_bitwidths: Levels, model,
                      group_id: int, layer_id: int, direction: str = "decrease") -> Optional[float]:
    """:67-107: decrease -> the highest available bitwidth below the current one; increase -> the lowest one above it
    that keeps the whole configuration within target_bits.  None when there is none."""
    layer_name = grouped_layer_names[group_id][layer_id]
    current_bw = current_bitwidths[group_id][layer_id]
    if direction == "decrease":
        candidates = [bw for bw, _ in available_bitwidths[layer_name] if bw < current_bw]
        return candidates[-1] if candidates else None
    candidates = [bw for bw, _ in available_bitwidths[layer_name] if bw > current_bw]
    if not candidates:
        return None
    numel = layer_numel(model, layer_name)
    current_total_bits = calculate_total_bits(current_bitwidths, grouped_layer_names, model)
    for bw in candidates:
        if current_total_bits + numel * (bw - current_bw) <= target_bits:
            return bw
    return None


class _Ctx:
    """The arguments every step of the search shares."""

    def __init__(self, model, grouped_layer_names, available_bitwidths: Levels, target_bits):
        self.model, self.names, self.levels, self.target_bits = model, grouped_layer_names, available_bitwidths, target_bits
        self.weights = [len(g) for g in grouped_layer_names]

    def next_bw(self, state, g, i, direction):
        return get_next_bitwidth(state, self.target_bits, self.names, self.levels, self.model, g, i, direction)

    def ids(self, state, g, direction) -> List[int]:
        return [i for i in range(len(self.names[g])) if self.next_bw(state, g, i, direction) is not None]

    def pick_group(self, rng: random.Random) -> int:
        return rng.choices(range(len(self.names)), weights=self.weights)[0]

    def bits(self, state):
        return calculate_total_bits(state, self.names, self.model)


def _decrease_to_budget(state: State, ctx: _Ctx, rng: random.Random, max_iterations: int) -> None:
    """:435-464 / :520-549 / :635-663: lower random layers, one level at a time, until the budget holds."""
    bits, iterations = ctx.bits(state), 0
    while bits > ctx.target_bits and iterations < max_iterations:
        iterations += 1
        g = ctx.pick_group(rng)
        decr_ids = ctx.ids(state, g, "decrease")
        if len(decr_ids) == 0:
            break
        i = rng.choice(decr_ids)
        state[g][i] = ctx.next_bw(state, g, i, "decrease")
        bits = ctx.bits(state)


# ------------------------------------------------------------------------------------------------ initialisation
def initial_parent(ctx: _Ctx, target_bitwidth: float) -> State:
    """:402-417, an integer target: that bitwidth where a layer has it, else the closest one it has."""
    parent = []
    for group_names in ctx.names:
        row = []
        for layer_name in group_names:
            bws = [bw for bw, _ in ctx.levels[layer_name]]
            row.append(target_bitwidth if target_bitwidth in bws else min(bws, key=lambda x: abs(x - target_bitwidth)))
        parent.append(row)
    return parent


def initial_candidates(ctx: _Ctx, target_bitwidth: float, initially_generated: int, rng: random.Random) -> List[State]:
    """:419-466, a fractional target: start every layer at the level closest to ceil(target) and lower random layers
    until the budget holds."""
    candidates = []
    for _ in range(initially_generated):
        candidate = [[min((bw for bw, _ in ctx.levels[n]), key=lambda x: abs(x - math.ceil(target_bitwidth))) for n in g]
                     for g in ctx.names]
        _decrease_to_budget(candidate, ctx, rng, 1000)
        candidates.append(candidate)
    return candidates


# ------------------------------------------------------------------------------------------------ mutation
def mutate(parent: State, rng: random.Random, ctx: _Ctx, group_rule: str) -> Optional[State]:
    """One offspring of `parent` (:513-742), or None where the reference `continue`s without one (no mutation
    succeeded).  The parent is not modified."""
    offspring = copy.deepcopy(parent)
    num_flips = min(rng.randint(1, 3), rng.randint(1, 3))  # bias towards lower values
    if group_rule == "none":  # there can be mutations between layers of different sizes
        _decrease_to_budget(offspring, ctx, rng, 1000)
        successful_increases = decrease_attempts = 0
        for _ in range(num_flips):
            g = ctx.pick_group(rng)
            incr_ids = ctx.ids(offspring, g, "increase")
            if len(incr_ids) == 0:  # make room: up to three decreases anywhere
                for _ in range(3):
                    decrease_attempts += 1
                    dg = ctx.pick_group(rng)
                    decr_ids = ctx.ids(offspring, dg, "decrease")
                    if decr_ids:
                        di = rng.choice(decr_ids)
                        offspring[dg][di] = ctx.next_bw(offspring, dg, di, "decrease")
                        incr_ids = ctx.ids(offspring, g, "increase")
                        if incr_ids:
                            break
            if incr_ids:
                i = rng.choice(incr_ids)
                offspring[g][i] = ctx.next_bw(offspring, g, i, "increase")
                successful_increases += 1
        if successful_increases == 0 and decrease_attempts > 5:
            return None
        return offspring
    # only mutations between layers of the same size / type
    if ctx.bits(offspring) > ctx.target_bits:
        _decrease_to_budget(offspring, ctx, rng, 100)
    successful_mutations = 0
    for _ in range(num_flips):
        g = ctx.pick_group(rng)
        decr_ids = ctx.ids(offspring, g, "decrease")
        if len(decr_ids) == 0:
            continue
        decr_id = rng.choice(decr_ids)
        incr_ids = ctx.ids(offspring, g, "increase")
        if len(incr_ids) == 0:  # lower another layer of the group first to make room
            other = rng.choice([i for i in decr_ids if i != decr_id]) if len(decr_ids) > 1 else None
            if other is not None:
                offspring[g][other] = ctx.next_bw(offspring, g, other, "decrease")
                incr_ids = ctx.ids(offspring, g, "increase")
            if len(incr_ids) == 0:
                continue
        incr_id = rng.choice(incr_ids)
        offspring[g][decr_id] = ctx.next_bw(offspring, g, decr_id, "decrease")
        offspring[g][incr_id] = ctx.next_bw(offspring, g, incr_id, "increase")
        successful_mutations += 1
    return offspring if successful_mutations else None


def make_offspring(parent: State, num_offspring: int, rng: random.Random, ctx: _Ctx, group_rule: str) -> List[State]:
    """:509-756: mutate until num_offspring distinct offspring, none equal to the parent, exist; more than ten duplicates
    in a row end the generation's list early."""
    offspring_list, duplicate_ct = [], 0
    while len(offspring_list) < num_offspring:
        offspring = mutate(parent, rng, ctx, group_rule)
        if offspring is None:
            continue
        if offspring in offspring_list or offspring == parent:
            duplicate_ct += 1
            if duplicate_ct > 10:
                break
            continue
        duplicate_ct = 0
        offspring_list.append(offspring)
    return offspring_list


# ------------------------------------------------------------------------------------------------ selection
def minibatch(calibration_data, num_tokens: int, rng: random.Random, fitness_fn: str = "ppl", target_logits=None):
    """:162-190: distinct random sequences holding exactly num_tokens tokens (the last one cut) -> (data, ids, targets);
    targets is None for `ppl`."""
    data, ids, targets, used = [], [], [], 0
    while used < num_tokens:
        i = rng.randint(0, len(calibration_data) - 1)
        if i in ids:
            continue
        ids.append(i)
        L = calibration_data[i].shape[1]
        if used + L > num_tokens:
            keep = num_tokens - used
            data.append(calibration_data[i][:, :keep])
            if fitness_fn == "kl":
                targets.append(target_logits[i][:, :keep])
            elif fitness_fn == "sparse_kl":
                targets.append((target_logits[i][0][:, :keep], target_logits[i][1][:, :keep]))
            used = num_tokens
        else:
            data.append(calibration_data[i])
            if fitness_fn in ("kl", "sparse_kl"):
                targets.append(target_logits[i])
            used += L
    return data, ids, (targets if targets else None)


def selection(evaluate: Callable, candidates: List[State], num_survive: int, calibration_data, num_tokens: int,
              rng: random.Random, fitness_fn: str = "ppl", target_logits=None, trace: Optional[list] = None, *,
              parent: Optional[State] = None, reuse=None, ranks=None):
    """:150-199: one minibatch, every candidate evaluated on it as evaluate(candidate, data, targets) -> float, the
    num_survive fittest kept -> (survivors, their fitnesses).

    ranks (suffix_forward.Ranks): the candidates are dealt to the ranks by cost (assign_candidates), each rank evaluates its
    share, and ONE all-gather of fp64 puts every fitness on every rank in candidate order.
    reuse (suffix_forward.StageReuse) and parent: this process's share is planned (plan_stage); where it reuses, the parent is
    captured on the minibatch and a candidate is evaluated as evaluate(candidate, data, targets, start_block).  Neither draws from rng nor
    changes the order of the list; with both absent this is the loop above."""
    data, ids, targets = minibatch(calibration_data, num_tokens, rng, fitness_fn, target_logits)
    if reuse is None and ranks is None:
        fitnesses = [evaluate(c, data, targets) for c in candidates]
    else:
        fitnesses = _evaluate_stage(evaluate, candidates, data, targets, parent, reuse, ranks)
    best_ids = np.argsort(fitnesses)[:num_survive]
    if trace is not None:
        trace.append({"num_tokens": num_tokens, "minibatch_ids": ids, "candidates": copy.deepcopy(candidates),
                      "fitnesses": [float(f) for f in fitnesses], "survivor_ids": [int(i) for i in best_ids]})
    return [candidates[i] for i in best_ids], [fitnesses[i] for i in best_ids]


def _evaluate_stage(evaluate: Callable, candidates: List[State], data, targets, parent, reuse, ranks) -> List[float]:
    """selection()'s fitness list with a stage plan and / or ranks: the same numbers in the same order.

    The candidate-to-rank map is computed from the candidates and the parent alone (reuse.costs: blocks from the first changed
    block; equal costs without reuse or parent), so it is the same on every rank.  What depends on a rank's free memory -- the
    stride, and whether reusing pays for ITS share -- is decided by that rank for itself after the map is fixed: a rank that
    declines runs its share in full, which gives the same numbers."""
    from .suffix_forward import assign_candidates
    world, rank = (ranks.world_size, ranks.rank) if ranks is not None else (1, 0)
    n = len(candidates)
    costs = reuse.costs(candidates, parent) if reuse is not None and parent is not None else [1.0] * n
    owner = assign_candidates(costs, world)
    mine = [i for i, r in enumerate(owner) if r == rank]
    starts = reuse.begin_stage([candidates[i] for i in mine], parent, data) if reuse is not None else None
    out, done = [0.0] * n, [0.0] * n
    try:
        if starts is not None:
            reuse.capture(parent, data)
        for k, i in enumerate(mine):
            c = candidates[i]
            out[i] = float(evaluate(c, data, targets) if starts is None else evaluate(c, data, targets, starts[k]))
            done[i] = 1.0
    finally:
        if reuse is not None:
            reuse.end_stage()
    if ranks is None:
        return out
    rows = ranks.gather(out + done)  # the one collective of the loop: every rank's fitnesses and which ones it computed
    for i in range(n):  # every candidate by its owner and by nobody else: the ranks agreed on the map
        who = [r for r in range(world) if rows[r][n + i] == 1.0]
        assert who == [owner[i]], f"candidate {i} belongs to rank {owner[i]} and was evaluated by ranks {who}"
    return [rows[owner[i]][i] for i in range(n)]


def search(ctx: _Ctx, evaluate: Callable, calibration_data, rng: random.Random, *, generations: int, offspring: int,
           target_bitwidth: float, survivors_per_selection: Sequence[int], tokens_per_selection: Sequence[int],
           group_rule: str = "size", fitness_fn: str = "ppl", target_logits=None, initially_generated: Optional[int] = None,
           initial_tokens: Optional[int] = None, on_generation: Optional[Callable] = None, reuse=None, ranks=None):
    """The loop of main() (:401-779) -> (final parent, its last train fitness, trace).  trace: one dict per generation,
    {"parent", "offspring", "stages": [selection's record per stage]} (and "initial" for a fractional target).
    on_generation(generation, parent, parent_bits, train_fitness) is called before each generation's offspring are made.
    reuse / ranks: handed to every selection() (the initial one of a fractional target has no parent and reuses nothing)."""
    assert len(survivors_per_selection) == len(tokens_per_selection), "Must have same number of stages"
    assert survivors_per_selection[-1] == 1, "Last stage should have only one survivor"
    trace = []
    if int(target_bitwidth) == target_bitwidth:
        parent, train_fitness = initial_parent(ctx, target_bitwidth), float("inf")
    else:
        assert initially_generated is not None, "Need initially_generated for non-integer initial level"
        assert initial_tokens is not None, "Need initial_tokens for non-integer initial level"
        stage = []
        cands, fits = selection(evaluate, initial_candidates(ctx, target_bitwidth, initially_generated, rng), 1,
                                calibration_data, initial_tokens, rng, fitness_fn, target_logits, stage, ranks=ranks)
        parent, train_fitness = cands[0], fits[0]
        trace.append({"initial": stage[0]})
    for generation in range(generations):
        if on_generation is not None:
            on_generation(generation, parent, ctx.bits(parent), train_fitness)
        offspring_list = make_offspring(parent, offspring, rng, ctx, group_rule)
        rec = {"parent": copy.deepcopy(parent), "offspring": copy.deepcopy(offspring_list), "stages": []}
        for num_survive, num_tokens in zip(survivors_per_selection, tokens_per_selection):
            if num_survive == survivors_per_selection[-1]:
                if parent not in offspring_list:  # elitist: the parent competes in the last stage
                    offspring_list.append(parent)
            offspring_list, train_fitnesses = selection(evaluate, offspring_list, num_survive, calibration_data, num_tokens,
                                                        rng, fitness_fn, target_logits, rec["stages"], parent=parent,
                                                        reuse=reuse, ranks=ranks)
        train_fitness, parent = train_fitnesses[0], offspring_list[0]
        trace.append(rec)
    return parent, train_fitness, trace


# ------------------------------------------------------------------------------------------------ output
def configuration_text(grouped_layer_names, parent: State, available_bitwidths: Levels) -> str:
    """:781-795: `name: bitwidth (filename)` per layer, groups in order, no trailing newline."""
    groups = ["\n".join(f"{n}: {bw} ({filename_of(available_bitwidths, n, bw)})" for n, bw in zip(names, bws))
              for names, bws in zip(grouped_layer_names, parent)]
    return "\n".join(groups)


def configuration_name(fitness_fn: str, target_bitwidth: float) -> str:
    return f"evo-{fitness_fn}-configuration-{target_bitwidth}.txt"


# ------------------------------------------------------------------------------------------------ the CLI
def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--model_name_or_path", type=str, required=True, help="The name or path to the model being searched")
    p.add_argument("--calibration_data", type=str, required=True, help=".pt file of [1, L] token-id tensors")
    p.add_argument("--calibration_tokens", default=524288, type=int, help="Number of tokens for calibration.")
    p.add_argument("--calibration_sequence_length", default=None, type=int, help="Length of calibration sequences.")
    p.add_argument("--eval_datasets", nargs="+", type=str, default=["fineweb_edu", "wikitext2", "c4"],
                   help=".pt files of [1, L] token-id tensors used for evaluation")
    p.add_argument("--eval_every", default=1, type=int, help="Eval every # generations.")
    p.add_argument("--eval_tokens", default=524288, type=int, help="Number of tokens for evaluation.")
    p.add_argument("--eval_sequence_length", default=None, type=int, help="Length of evaluation sequences.")
    p.add_argument("--fitness_fn", choices=["ppl", "kl", "sparse_kl"], default="kl", help="Fitness function.")
    p.add_argument("--log_wandb", default=False, action="store_true", help="Whether to log to W&B")
    p.add_argument("--generations", type=int, required=True, help="Number of generations in evolutionary search")
    p.add_argument("--offspring", type=int, required=True, help="Number of offspring generated in each generation")
    p.add_argument("--target_bitwidth", type=float, required=True,
                   help="Base level for all layers. If no integer, initialize random with this average")
    p.add_argument("--quant_weights_path", type=str, required=True, help="Path to quantized weights")
    p.add_argument("--survivors_per_selection", type=int, nargs="+", required=True,
                   help="Number of survivors after each stage of selection")
    p.add_argument("--tokens_per_selection", type=int, nargs="+", required=True,
                   help="Number of calibration tokens at each stage of selection")
    p.add_argument("--initially_generated", type=int,
                   help="Only for non-integer initial level: number of search points generated in the beginning")
    p.add_argument("--initial_tokens", type=int,
                   help="Only for non-integer initial level: number of calibration tokens used for the initial generation")
    p.add_argument("--group_rule", type=str, default="size", choices=["size", "name", "none"],
                   help="Layer grouping rule. Mutations are performed only within a group.")
    p.add_argument("--kl_topk", type=int, default=10, help="TopK logits in KL-divergence (for sparse_kl fitness function)")
    p.add_argument("--dtype", type=str, default="auto", choices=["auto", "float16", "float32", "bfloat16"],
                   help="dtype to load the model.")
    p.add_argument("--seed", default=0, type=int, help="Random seed.")
    p.add_argument("--attn_implementation", type=str, default=None, choices=["eager", "sdpa", "flash_attention_2"],
                   help="Attention implementation: eager, sdpa, or flash_attention_2")
    p.add_argument("--targets_on", type=str, default="device", choices=["cpu", "device"],
                   help="where the KL targets are kept: on the device when they fit (default), or on the host as the reference")
    p.add_argument("--resident", type=str, default="dense", choices=["dense", "packed"],
                   help="dense (default): the model keeps a dense live weight per Linear and a switch decodes into it; packed: "
                        "no dense copy, the forward reads the stored block bytes (fp16 / bf16 models, packed levels)")
    p.add_argument("--moe_prefill", type=str, default="loop", choices=["loop", "grouped"],
                   help="with --resident packed: how the packed experts of a MoE model take more than a decode step's tokens "
                        "(PackedExperts.prefill)")
    p.add_argument("--reuse_prefix", type=str, default="off", choices=["off", "on"],
                   help="on: run the parent once per minibatch and evaluate every candidate from its first changed block "
                        "(suffix_forward); the trajectory is the one of `off`")
    p.add_argument("--reuse_prefix_bytes", type=int, default=None,
                   help="device memory the cached hidden states may take (default: what is free, less a reserve)")
    p.add_argument("--backend", type=str, default=None, choices=["nccl", "gloo"],
                   help="under torch.distributed.run: nccl (= RCCL; default with one GPU per rank) or gloo (default "
                        "otherwise: the ranks share the visible GPUs)")
    p.add_argument("--trace_out", type=str, default=None, help="write search()'s trace to this file as JSON (rank 0)")
    p.add_argument("--report_out", type=str, default=None,
                   help="write the report of the final configuration -- ppl_eval/<dataset>, ppl_train, train_fitness, in full "
                        "precision -- to this file as JSON (rank 0)")
    args = p.parse_args(argv)
    # every refusal BEFORE any work
    for what, names in (("calibration_data", [args.calibration_data]), ("eval_datasets", args.eval_datasets)):
        for name in names:
            if not os.path.isfile(name):
                p.error(f"{what} must be a .pt file of token-id tensors (got {name!r}); dataset downloads are not part of "
                        "this package")
    if not os.path.isdir(args.quant_weights_path):
        p.error(f"quant_weights_path {args.quant_weights_path!r} is not a directory")
    if len(args.survivors_per_selection) != len(args.tokens_per_selection):
        p.error("survivors_per_selection and tokens_per_selection must have the same number of stages")
    if args.survivors_per_selection[-1] != 1:
        p.error("the last stage must have exactly one survivor")
    if int(args.target_bitwidth) != args.target_bitwidth and (args.initially_generated is None or args.initial_tokens is None):
        p.error("a non-integer target_bitwidth needs --initially_generated and --initial_tokens")
    if args.log_wandb:
        try:
            import wandb  # noqa: F401
        except ModuleNotFoundError:
            p.error("--log_wandb: `wandb` is not installed")
    return args


def compute_fitness(model, data, fitness_fn: str, target_logits=None, logits_fn=None) -> float:
    """:141-147.  logits_fn: metrics' way to take a sequence's logits from something other than model(inputs)."""
    from . import metrics
    if fitness_fn == "ppl":
        return metrics.compute_perplexity(model, data, logits_fn=logits_fn)
    if fitness_fn == "kl":
        return metrics.compute_kl_div(model, data, target_logits, logits_fn=logits_fn)
    return metrics.compute_sparse_kl_div(model, data, target_logits, logits_fn=logits_fn)


def suffix_evaluate(store, runner, model, fitness_fn: str) -> Callable:
    """evaluate(candidate, data, targets[, start_block]) on a level store: the plain evaluation, or with start_block the
    logits of every sequence from the runner's cached boundary."""
    def evaluate(candidate, data, targets, start_block=None):
        store.switch(candidate)
        if start_block is None:
            return compute_fitness(model, data, fitness_fn, targets)
        return compute_fitness(model, data, fitness_fn, targets,
                               logits_fn=lambda i, inputs: runner.logits(i, start_block, inputs))
    return evaluate


def sharded_perplexity(model, data, ranks) -> float:
    """compute_perplexity with the sequences dealt to the ranks (sequence i to rank i % world_size): every rank sums the
    fp32 per-row NLL of its share in fp64, one gather of (sum, rows) per rank, exp(total / rows).  Reporting only: the last
    digits may differ from one rank's compute_perplexity (another order of the fp64 sum)."""
    import torch
    from . import metrics
    mine = data[ranks.rank::ranks.world_size]
    rows = metrics.nll_rows(model, mine)
    parts = ranks.gather([float(rows.sum(dtype=torch.float64).item()), float(rows.numel())])
    return math.exp(sum(p[0] for p in parts) / sum(p[1] for p in parts))


def init_ranks(backend: Optional[str]):
    """Under torch.distributed.run: join the process group -> (Ranks, device); otherwise (None, cuda)."""
    import torch
    if "RANK" not in os.environ or not torch.distributed.is_available():
        return None, torch.device("cuda")
    import torch.distributed as dist
    from .suffix_forward import Ranks
    world, local = int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", os.environ["RANK"]))
    own_gpu = torch.cuda.device_count() >= int(os.environ.get("LOCAL_WORLD_SIZE", world))
    backend = backend or ("nccl" if own_gpu else "gloo")
    device = torch.device("cuda", local if own_gpu else local % torch.cuda.device_count())
    torch.cuda.set_device(device)
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=device)  # nccl == RCCL on ROCm
    else:
        dist.init_process_group("gloo")
    return Ranks(device if backend == "nccl" else "cpu"), device


def collect_targets(model, calibration_data, fitness_fn: str, kl_topk: int, targets_on: str, reserve_bytes: int = 0):
    """The KL targets of the unmodified model (:360-373) -> (list, "device" | "cpu").  Dense targets stay on the device
    only when all of them fit in the memory that is free now, less reserve_bytes; otherwise each one is moved to the
    host as it is produced."""
    import torch
    from . import metrics
    if fitness_fn == "ppl":
        return [], targets_on
    device = next(model.parameters()).device
    if targets_on == "device" and fitness_fn == "kl" and device.type == "cuda":
        es = next(model.parameters()).element_size()
        need = sum(ids.shape[0] * ids.shape[1] for ids in calibration_data) * model.config.vocab_size * es
        if need + reserve_bytes > torch.cuda.mem_get_info(device)[0]:
            targets_on = "cpu"
    out = []
    for ids in calibration_data:
        t = metrics.collect_target_logits(model, [ids], topk=kl_topk if fitness_fn == "sparse_kl" else None)[0]
        if targets_on == "cpu":
            t = tuple(x.cpu() for x in t) if isinstance(t, tuple) else t.cpu()
        out.append(t)
    return out, targets_on


def main(argv=None):
    args = parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "evo_quant_search needs a GPU (there is no CPU path)"
    ranks, device = init_ranks(args.backend)
    try:
        return _run(args, ranks, device)
    finally:  # also when the run raises: the launcher then reports the real error, not a hung rendezvous
        if ranks is not None:
            torch.distributed.destroy_process_group()


def _run(args, ranks, device):
    """Every rank loads the model, builds its own level store, holds all targets and seeds the same random.Random: the host
    decisions of the trajectory are replicated (a rank's cache stride is its own and decides nothing shared: _evaluate_stage).
    Rank 0 alone prints the report, logs and writes."""
    import json
    import torch
    from . import metrics
    from . import dist_utils
    from .level_store import LevelStore, default_layer_names
    from .ppleval import load_hf_model
    main_rank = ranks is None or ranks.rank == 0
    say = dist_utils.print_on_main  # every line of the run's report is rank 0's
    metrics.fix_seed(args.seed)
    rng = random.Random(args.seed)
    if args.log_wandb and main_rank:
        import wandb
        wandb.init(config=args)
    model = load_hf_model(args, device)
    max_len = min(model.config.max_position_embeddings, 8192)
    args.calibration_sequence_length = args.calibration_sequence_length or max_len
    args.eval_sequence_length = args.eval_sequence_length or max_len
    calibration_data = metrics.load_eval_data(args.calibration_data, args.calibration_tokens,
                                              args.calibration_sequence_length, what="calibration_data")
    eval_datasets = [metrics.load_eval_data(n, args.eval_tokens, args.eval_sequence_length) for n in args.eval_datasets]

    # the levels: HF-named directories as the reference scans them, else the model's Linears through layer_dir
    available = scan_available_bitwidths(args.quant_weights_path)
    if not available or not all(_is_module(model, n) for n in available):
        names = default_layer_names(model, args.quant_weights_path)  # Linears, and the units of fused experts modules
        # a database cut from a whole model also holds output.weight: lm_head is no Linear of a block (layer_order_fn has
        # no place for it) and is not searched -- it keeps the model's own weights
        outside = [n for n in names if not _in_a_block(n)]
        if outside:
            say(f"not searched (no Linear of a block): {outside}")
        names = [n for n in names if n not in outside]
        available = scan_available_bitwidths(args.quant_weights_path, names)
    say("Available bitwidths:")
    for layer_name, bitwidths in available.items():
        say(f"{layer_name}: {[bw for bw, _ in bitwidths]}")
    layer_names = sorted(available, key=layer_order_fn)
    grouped = group_layers(model, layer_names, args.group_rule)
    say(grouped)
    if args.resident == "packed":  # the targets need the unmodified dense model: first, before the store frees it
        target_logits, where = collect_targets(model, calibration_data, args.fitness_fn, args.kl_topk, args.targets_on)
    # refuses what does not fit before uploading
    store = LevelStore(model, args.quant_weights_path, device, layer_names, resident=args.resident,
                       moe_prefill=args.moe_prefill)
    store.grouped_layer_names = grouped
    say(f"level store: {store.bytes()} bytes on {device}" +
          (f", {store.freed_bytes} bytes of dense weights freed" if args.resident == "packed" else ""))
    if args.resident != "packed":
        target_logits, where = collect_targets(model, calibration_data, args.fitness_fn, args.kl_topk, args.targets_on)
    if args.fitness_fn != "ppl":
        say(f"targets on: {where}")

    ctx = _Ctx(model, grouped, available, target_bits_of(grouped, model, args.target_bitwidth))
    quantizable_weights = sum(layer_numel(model, n) for n in layer_names)
    log_dict = {}

    reuse = runner = None
    if args.reuse_prefix == "on":
        from .suffix_forward import StageReuse, SuffixRunner
        # (a stage that does not fit is a rank's own finding: that message comes from the rank it concerns)
        log = say if ranks is None else (lambda msg: print(f"[rank {ranks.rank}] {msg}"))
        runner = SuffixRunner(model, budget_bytes=args.reuse_prefix_bytes, log=log)
        reuse = StageReuse(runner, store)
    evaluate = suffix_evaluate(store, runner, model, args.fitness_fn)

    def perplexity(data):
        return metrics.compute_perplexity(model, data) if ranks is None else sharded_perplexity(model, data, ranks)

    def evaluate_parent(tag=""):  # (the store's state is the caller's; a stage's cache never outlives its stage)
        for name, data in zip(args.eval_datasets, eval_datasets):
            ppl = perplexity(data)
            say(f"{name}: {ppl:.2f}")
            log_dict[f"ppl_eval/{name}"] = ppl
        ppl_train = perplexity(calibration_data)
        say(f"ppl_train: {ppl_train:.2f}")
        log_dict["ppl_train"] = ppl_train

    def on_generation(generation, parent, parent_bits, train_fitness):
        say(f"Generation {generation + 1}/{args.generations}")
        say("Current search point:")
        for group in parent:
            say(group)
        say(f"Parent bits: {parent_bits}")
        say(f"Bit average: {parent_bits / quantizable_weights:.4e}")
        say(f"Train fitness: {train_fitness:.4e}")
        if runner is not None:
            runner.invalidate()
        store.switch(parent)
        if generation % args.eval_every == 0:
            evaluate_parent()
        if args.log_wandb and main_rank:
            wandb.log(log_dict)

    parent, train_fitness, trace = search(
        ctx, evaluate, calibration_data, rng, generations=args.generations, offspring=args.offspring,
        target_bitwidth=args.target_bitwidth, survivors_per_selection=args.survivors_per_selection,
        tokens_per_selection=args.tokens_per_selection, group_rule=args.group_rule, fitness_fn=args.fitness_fn,
        target_logits=target_logits, initially_generated=args.initially_generated, initial_tokens=args.initial_tokens,
        on_generation=on_generation, reuse=reuse, ranks=ranks)
    log_dict["train_fitness"] = train_fitness
    if reuse is not None:
        say(f"reuse_prefix: {sum(st[0] for st in reuse.stages)} of {len(reuse.stages)} stages reused the parent's prefix "
              f"({runner.captures} captures on this rank)")
    out = os.path.join(args.quant_weights_path, configuration_name(args.fitness_fn, args.target_bitwidth))
    if main_rank:  # to a temporary name, then renamed: no reader sees half a file
        with open(out + ".tmp", "w") as f:
            f.write(configuration_text(grouped, parent, available))
        os.replace(out + ".tmp", out)
        if args.trace_out:
            with open(args.trace_out + ".tmp", "w") as f:
                json.dump(trace, f)
            os.replace(args.trace_out + ".tmp", args.trace_out)
    say("Final configuration:")
    for group in parent:
        say(group)
    store.switch(parent)
    evaluate_parent()
    if args.log_wandb and main_rank:
        wandb.log(log_dict)
    if args.report_out and main_rank:
        with open(args.report_out + ".tmp", "w") as f:
            json.dump(log_dict, f)
        os.replace(args.report_out + ".tmp", args.report_out)
    return parent, out


def _in_a_block(name: str) -> bool:
    try:
        layer_order_fn(name)
        return True
    except (IndexError, ValueError):
        return False


def _is_module(model, name) -> bool:
    try:
        return hasattr(model.get_submodule(name), "weight")
    except AttributeError:
        return False


if __name__ == "__main__":
    main()
