#!/usr/bin/env python3
"""Seconds per generation of evo_quant_search.search on one GPU: --reuse_prefix on against off, dense and packed residency.

    python profiles/search_scale.py --blocks 8 --resident dense packed --reuse off on --reps 3 --out search_scale.json

A random-init model of Llama-3-8B's shape (hidden 4096, intermediate 14336, 32 / 8 heads, vocabulary 128256) with --blocks
decoder blocks in bf16, three RTN levels per Linear (Q2_K, Q4_K, Q6_K as "2", "4", "6") written to a --gguf-layers database
on the fly (kept in --db between calls), random token ids, KL fitness against the unmodified model.  Offspring 32, stages
(4, 1) x (2048, 16384) tokens, sequences of 8192 tokens, one seed: `on` and `off` walk the same candidates.

Per residency: one untimed generation of every variant (all shapes warm), then --reps repetitions that ALTERNATE the variants;
a repetition is --generations generations between two device synchronisations.  Reported per variant: every repetition's
seconds per generation, the median, min and max; for `on` the plan's predicted saving (block forwards avoided / block
forwards of the plain loop, the capture charged) and whether the trace equals `off`'s.  The GPU's clocks are read, never set.

--root DIR puts another checkout of the package first on sys.path (the parent commit, for the `off` path); `--reuse off`
uses nothing that a checkout without suffix_forward lacks."""
import argparse
import copy
import json
import os
import random
import re
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
LEVELS = ((10, "2"), (12, "4"), (14, "6"))
LINEARS = r"((q|k|v|o|gate|up|down)_proj)$"


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=60).stdout
        return [ln.strip() for ln in out.splitlines() if re.search(r"GPU\[0\].*(sclk|mclk|Power)", ln)]
    except (OSError, subprocess.TimeoutExpired) as e:
        return [f"rocm-smi: {e}"]


def build_model(torch, blocks):
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=blocks, num_attention_heads=32,
                      num_key_value_heads=8, vocab_size=128256, max_position_embeddings=8192, rms_norm_eps=1e-5,
                      rope_theta=500000.0, tie_word_embeddings=False, attn_implementation="sdpa", use_cache=False)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = LlamaForCausalLM(cfg)
    return model.to(torch.bfloat16).eval()


def write_db(torch, ops, model, names, db):
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import map_tensor_name
    for n in names:
        W = model.get_submodule(n).weight.data
        g = map_tensor_name(n + ".weight")
        os.makedirs(os.path.join(db, g), exist_ok=True)
        for t, num in LEVELS:
            packed = ops.pack(t, *ops.rtn_quantize(W, t))
            packed.cpu().numpy().tofile(os.path.join(db, g, f"{num}.pth"))
            with open(os.path.join(db, g, f"{num}-metadata.json"), "w") as f:
                json.dump({"tensor_info": {"name": g, "type": t, "shape": [W.shape[1], W.shape[0]],
                                           "np_shape": list(packed.shape), "np_dtype": "uint8"}}, f)
    md = {"general.architecture": {"value": "llama"}, "llama.attention.head_count": {"value": 32},
          "llama.attention.head_count_kv": {"value": 8}}
    with open(os.path.join(db, "manifest.json"), "w") as f:
        json.dump({"metadata": md}, f)


def predicted_saving(stages, n_blocks):
    """(block forwards of the plain loop, block forwards with the plan, the capture included) over all planned stages."""
    plain = with_plan = 0
    for reused, _, starts in stages:
        plain += n_blocks * len(starts)
        with_plan += (n_blocks + sum(n_blocks - s for s in starts)) if reused else n_blocks * len(starts)
    return plain, with_plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--resident", nargs="+", default=["dense", "packed"], choices=["dense", "packed"])
    ap.add_argument("--reuse", nargs="+", default=["off", "on"], choices=["off", "on"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--generations", type=int, default=2)
    ap.add_argument("--offspring", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--db", default=os.path.join(tempfile.gettempdir(), "search_scale_db"))
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose package is measured")
    ap.add_argument("--out", default="search_scale.json")
    ap.add_argument("--breakdown", action="store_true",
                    help="synchronise around every evaluation and capture and report the seconds per stage size")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import gptq_gguf_toolkit_amd
    from gptq_gguf_toolkit_amd import evo_quant_search as S, metrics, ops
    from gptq_gguf_toolkit_amd.level_store import LevelStore
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    result = {"package": os.path.dirname(os.path.abspath(gptq_gguf_toolkit_amd.__file__)), "args": vars(args),
              "device": torch.cuda.get_device_name(0), "clocks_before": clocks(), "runs": []}

    def save():
        with open(args.out + ".tmp", "w") as f:
            json.dump(result, f, indent=1)
        os.replace(args.out + ".tmp", args.out)

    base = build_model(torch, args.blocks)
    names = [n for n, m in base.named_modules() if isinstance(m, torch.nn.Linear) and re.search(LINEARS, n)]
    db = f"{args.db}_{args.blocks}"
    if not os.path.isfile(os.path.join(db, "manifest.json")):
        t0 = time.perf_counter()
        write_db(torch, ops, base, names, db)
        print(f"level database of {len(names)} Linears written in {time.perf_counter() - t0:.1f} s", flush=True)
    g = torch.Generator().manual_seed(1)
    calib = [torch.randint(0, 128256, (1, 8192), generator=g) for _ in range(4)]
    targets = metrics.collect_target_logits(base, calib)
    kw = dict(offspring=args.offspring, target_bitwidth=4.0, survivors_per_selection=(4, 1),
              tokens_per_selection=(2048, 16384), group_rule="size", fitness_fn="kl", target_logits=targets)

    for resident in args.resident:
        model = copy.deepcopy(base)
        levels = S.scan_available_bitwidths(db, names)
        grouped = S.group_layers(model, sorted(levels, key=S.layer_order_fn), "size")
        store = LevelStore(model, db, "cuda", [n for gr in grouped for n in gr], resident=resident)
        store.grouped_layer_names = grouped
        ctx = S._Ctx(model, grouped, levels, S.target_bits_of(grouped, model, 4.0))

        def run(reuse_prefix, generations):
            extra, reuse = {}, None
            if reuse_prefix == "on":
                from gptq_gguf_toolkit_amd.suffix_forward import StageReuse, SuffixRunner
                runner = SuffixRunner(model, log=lambda *a: None)
                reuse = StageReuse(runner, store)
                evaluate = S.suffix_evaluate(store, runner, model, "kl")
                extra = {"reuse": reuse}
            else:
                def evaluate(candidate, data, tg):
                    store.switch(candidate)
                    return S.compute_fitness(model, data, "kl", tg)
            parts = {}
            if args.breakdown:
                def timed(fn, what):
                    def call(*a, **k):
                        torch.cuda.synchronize()
                        t = time.perf_counter()
                        out = fn(*a, **k)
                        torch.cuda.synchronize()
                        key = f"{what} {sum(int(x.shape[1]) for x in (a[1] if what == 'evaluate' else a[0]))} tokens"
                        parts[key] = parts.get(key, 0.0) + (time.perf_counter() - t) / generations
                        return out
                    return call
                evaluate = timed(evaluate, "evaluate")
                if reuse is not None:
                    runner.capture = timed(runner.capture, "capture")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, trace = S.search(ctx, evaluate, calib, random.Random(args.seed), generations=generations, **kw, **extra)
            torch.cuda.synchronize()
            if parts:
                print(f"  {reuse_prefix}: " + ", ".join(f"{k} {v:.3f} s" for k, v in sorted(parts.items())), flush=True)
            return (time.perf_counter() - t0) / generations, trace, reuse

        for v in args.reuse:  # every shape of every variant once, untimed
            t, _, _ = run(v, 1)
            print(f"{resident} {v}: warm-up generation {t:.2f} s", flush=True)
        times, traces, plans = {v: [] for v in args.reuse}, {}, {}
        for rep in range(args.reps):
            for v in args.reuse:  # alternate
                t, trace, reuse = run(v, args.generations)
                times[v].append(t)
                traces[v] = trace
                if reuse is not None:
                    plans[v] = (predicted_saving(reuse.stages, args.blocks), sum(st[0] for st in reuse.stages), len(reuse.stages))
                print(f"{resident} {v} rep {rep}: {t:.3f} s per generation", flush=True)
        for v in args.reuse:
            rec = {"resident": resident, "reuse_prefix": v, "s_per_generation": times[v],
                   "median": statistics.median(times[v]), "min": min(times[v]), "max": max(times[v]),
                   "candidates_evaluated": sum(len(st["candidates"]) for r in traces[v] for st in r["stages"])}
            if v in plans:
                (plain, with_plan), reused, stages = plans[v]
                rec.update(block_forwards_plain=plain, block_forwards_with_plan=with_plan,
                           predicted_saving=1 - with_plan / plain, stages_reused=f"{reused} of {stages}")
            if v == "on" and "off" in traces:
                rec["trace_equals_off"] = traces["on"] == traces["off"]
            result["runs"].append(rec)
            print(json.dumps(rec), flush=True)
        result["clocks_after_" + resident] = clocks()
        save()
        del store, model, ctx
        torch.cuda.empty_cache()
    save()


if __name__ == "__main__":
    main()
