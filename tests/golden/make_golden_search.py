#!/usr/bin/env python3
"""G19: the trajectory of the reference's bit-width search, by RUNNING THE REFERENCE's main() (read-only at
/root/reference/evopress/evo_quant_search.py) on the CPU with everything around the loop replaced by stand-ins:
  model    : three blocks of seven bias-free nn.Linear layers (tiny shapes, the size classes of a Llama block) behind
             AutoModelForCausalLM.from_pretrained; tokenizer: none
  database : a temporary directory of torch-saved zero tensors, five levels per layer, which the reference's own
             scan_available_bitwidths / load_layers read
  data     : twelve [1, 64] id tensors behind get_data
  fitness  : compute_perplexity replaced by FITNESS below, a fixed function of model.state (the configuration that
             load_layers has just made current); every call with a selection minibatch is recorded
for one seed per group rule.  Recorded per rule: every evaluated candidate in order, as a [n, 21] fp64 array of bitwidths
(layers in grouped order), and the bytes of the configuration file main() wrote -- tests/golden/G19_search.npz.
`ours(rule)` drives this package's evo_quant_search.search on the same problem; tests/test_search_cpu.py demands the
identical sequence.  Nothing of the reference is copied.  `python make_golden_search.py` runs only where the reference is;
the tests read the fixture and call ours()."""
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/evopress"
BWS = [(2.5625, "2.5625-Q2_K.pth"), (3.4375, "3.4375-Q3_K.pth"), (4.5, "4.5-Q4_K.pth"), (5.5, "5.5-Q5_K.pth"),
       (6.5625, "6.5625-Q6_K.pth")]
SHAPES = {"self_attn.q_proj": (8, 8), "self_attn.k_proj": (2, 8), "self_attn.v_proj": (2, 8), "self_attn.o_proj": (8, 8),
          "mlp.gate_proj": (16, 8), "mlp.up_proj": (16, 8), "mlp.down_proj": (8, 16)}
BLOCKS = 3
# rule -> (seed, target_bitwidth, initially_generated, initial_tokens): an integer target that is no level (the first parent
# is above the budget), and fractional ones (the initial population path)
RUNS = {"size": (5, 3.7, 4, 128), "name": (6, 4.0, None, None), "none": (7, 3.9, 3, 192)}
GENERATIONS, OFFSPRING, SURVIVORS, TOKENS = 5, 8, (3, 1), (100, 200)


def layer_names():
    return [f"model.layers.{b}.{k}" for b in range(BLOCKS) for k in SHAPES]


def calib():
    return [torch.full((1, 64), i, dtype=torch.long) for i in range(12)]


def fitness_of(flat_bitwidths):
    """A fixed function of the state: sum over layers (in sorted-name order) of weight x numel x 2^-bitwidth."""
    total = 0.0
    for i, (name, bw) in enumerate(sorted(flat_bitwidths.items())):
        r, c = SHAPES[name.split(".", 3)[3]]
        total += (1.0 + 0.37 * ((7 * i) % 5)) * r * c * 2.0 ** (-bw)
    return total


class StubModel(torch.nn.Module):

    def __init__(self):
        super().__init__()
        self.config = types.SimpleNamespace(use_cache=True, max_position_embeddings=64)
        self.model = torch.nn.Module()
        self.model.layers = torch.nn.ModuleList()
        for _ in range(BLOCKS):
            blk = torch.nn.Module()
            blk.self_attn, blk.mlp = torch.nn.Module(), torch.nn.Module()
            for k, (r, c) in SHAPES.items():
                sub, leaf = k.split(".")
                setattr(getattr(blk, sub), leaf, torch.nn.Linear(c, r, bias=False))
            self.model.layers.append(blk)


def reference(rule):
    """-> (states [n, 21], configuration file bytes) from the reference's main()."""
    sys.path.insert(0, REF)
    import evo_quant_search as R
    seed, target, init_n, init_tokens = RUNS[rule]
    data, recorded = calib(), []
    with tempfile.TemporaryDirectory() as db:
        model = StubModel()
        for n in layer_names():
            os.makedirs(os.path.join(db, n))
            for _, f in BWS:
                torch.save(torch.zeros_like(model.get_submodule(n).weight), os.path.join(db, n, f))
        grouped = {}

        def ppl(m, d):
            names = [n for g in grouped["names"] for n in g]
            flat = dict(zip(names, [bw for g in m.state for bw in g]))
            if d is not data:  # a selection minibatch (the evaluation passes hand the calibration list itself)
                recorded.append([flat[n] for n in names])
            return fitness_of(flat)

        real_group = R.group_layers

        def group_layers(m, names, group_rule):
            grouped["names"] = real_group(m, names, group_rule)
            return grouped["names"]

        R.parse_args = lambda: types.SimpleNamespace(
            model_name_or_path="stub", tokenizer_name=None, calibration_data="stub", calibration_tokens=768,
            calibration_sequence_length=64, eval_datasets=[], eval_every=1, eval_tokens=0, eval_sequence_length=64,
            fitness_fn="ppl", log_wandb=False, generations=GENERATIONS, offspring=OFFSPRING, target_bitwidth=target,
            quant_weights_path=db, survivors_per_selection=list(SURVIVORS), tokens_per_selection=list(TOKENS),
            initially_generated=init_n, initial_tokens=init_tokens, group_rule=rule, kl_topk=10, dtype="float32", seed=seed,
            attn_implementation=None, use_fast_tokenizer=False)
        R.AutoModelForCausalLM = types.SimpleNamespace(from_pretrained=lambda *a, **k: model)
        R.AutoTokenizer = types.SimpleNamespace(from_pretrained=lambda *a, **k: None)
        R.get_data = lambda *a, **k: data
        R.compute_perplexity = ppl
        R.group_layers = group_layers
        R.main()
        with open(os.path.join(db, f"evo-ppl-configuration-{target}.txt"), "rb") as f:
            text = f.read()
    return np.asarray(recorded, dtype=np.float64), text


def ours(rule):
    """-> (states, configuration text) from this package's search on the same problem."""
    from gptq_gguf_toolkit_amd import evo_quant_search as S
    seed, target, init_n, init_tokens = RUNS[rule]
    shapes = {n: SHAPES[n.split(".", 3)[3]] for n in layer_names()}
    model = types.SimpleNamespace(get_submodule=lambda n: types.SimpleNamespace(
        weight=types.SimpleNamespace(numel=lambda: shapes[n][0] * shapes[n][1])))
    levels = {n: list(BWS) for n in layer_names()}
    grouped = S.group_layers(model, sorted(levels, key=S.layer_order_fn), rule)
    ctx = S._Ctx(model, grouped, levels, S.target_bits_of(grouped, model, target))
    names, recorded = [n for g in grouped for n in g], []

    def evaluate(candidate, data, targets):
        flat = dict(zip(names, [bw for g in candidate for bw in g]))
        recorded.append([flat[n] for n in names])
        return fitness_of(flat)

    parent, _, _ = S.search(ctx, evaluate, calib(), random.Random(seed), generations=GENERATIONS, offspring=OFFSPRING,
                            target_bitwidth=target, survivors_per_selection=SURVIVORS, tokens_per_selection=TOKENS,
                            group_rule=rule, fitness_fn="ppl", initially_generated=init_n, initial_tokens=init_tokens)
    return recorded, S.configuration_text(grouped, parent, levels)


def main():
    out = {}
    for rule in RUNS:
        states, text = reference(rule)
        out[f"{rule}_states"] = states
        out[f"{rule}_config"] = np.frombuffer(text, dtype=np.uint8)
        print(rule, states.shape, len(text), "bytes of configuration")
    np.savez_compressed(os.path.join(HERE, "G19_search.npz"), **out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    main()
