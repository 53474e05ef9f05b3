#!/usr/bin/env python3
"""Perplexity of a model whose Linear weights come from a per-layer level database or from a `.gguf`: the reference's
eval/ppleval.py (:25-120 flags, :124-152 load_compressed_weights, :207-229 the result JSON) on the gq_eval_* kernels.

    python -m gptq_gguf_toolkit_amd.ppleval --model_name_or_path HF_DIR --eval_datasets ids.pt --output_file out.json \
        [--quant_weights_path DB [--quant_config_path FILE] [--quant_default_level N] | --gguf FILE [--packed [--packed_vocab] [--moe_prefill grouped]]] \
        [--kl_against none|model|gguf:FILE]

Evaluation data are `.pt` files of [1, L] id tensors (no tokenizer, no download).  Left out: --memory_efficient, wandb,
the sparse / drop-layer branches, the fast-tokenizer flag.  Beyond the reference: --gguf (weights decoded from the file by
gguf_loader) and --kl_against (dense KL of the scored model against the unmodified HF model or another .gguf; the target
is evaluated first and its logits stay on the device in the model dtype)."""
import argparse
import json
import os
import re
import sys

import torch

if __package__ in (None, ""):  # run as a script: make the package importable under its alias
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gptq_gguf_toolkit_amd  # noqa: F401
    __package__ = "gptq_gguf_toolkit_amd"

from . import gguf_loader, level_db, metrics  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    # Model params
    p.add_argument("--model_name_or_path", type=str, required=True, help="The name or path to the model being evaluated")
    # Data params
    p.add_argument("--sequence_length", default=None, type=int, help="Length of sequences.")
    p.add_argument("--eval_datasets", nargs="+", type=str, required=True,
                   help=".pt files of [1, L] token-id tensors used for evaluation")
    p.add_argument("--eval_batch_size", type=int, default=1, help="Batch size on evaluation")
    p.add_argument("--eval_tokens", default=524288, type=int, help="Number of tokens for evaluation.")
    # Quantization params
    p.add_argument("--quant_weights_path", type=str, default=None, help="Path to quantized weights")
    p.add_argument("--quant_config_path", type=str, default=None, help="Path to quantization config")
    p.add_argument("--quant_default_level", type=int, default=0, help="Default quantization level")
    # Output params
    p.add_argument("--output_file", type=str, required=True, help="Path to output JSON file for storing results")
    # Misc params
    p.add_argument("--dtype", type=str, default="float16", choices=["auto", "float16", "float32", "bfloat16"],
                   help="dtype to load the model.")
    p.add_argument("--seed", default=0, type=int, help="Random seed.")
    p.add_argument("--attn_implementation", type=str, default=None, choices=["eager", "sdpa", "flash_attention_2"],
                   help="Attention implementation: eager, sdpa, or flash_attention_2")
    # beyond the reference
    p.add_argument("--gguf", type=str, default=None, help="take ALL weights from this .gguf (decoded on the GPU)")
    p.add_argument("--kl_against", type=str, default="none",
                   help="none | model | gguf:FILE -- also report the dense KL of the scored model against the unmodified "
                        "HF model or against another .gguf")
    p.add_argument("--packed", default=False, action="store_true",
                   help="with --gguf: keep the K-quant / Q8_0 / IQ4_NL / IQ4_XS weights of the blocks' Linears packed on the device and compute "
                        "with the block bytes (no dense copy; fp16 / bf16)")
    p.add_argument("--packed_vocab", default=False, action="store_true",
                   help="with --packed: keep token_embd and output packed as well (a PackedEmbedding and a packed lm_head)")
    p.add_argument("--moe_prefill", type=str, default="loop", choices=["loop", "grouped"],
                   help="with --packed: how the packed experts of a MoE model take more than a decode step's tokens -- the "
                        "per-expert loop, or device-side routing and one grouped GEMM per projection")
    args = p.parse_args(argv)
    if args.packed and not args.gguf:
        p.error("--packed needs --gguf")
    if args.packed_vocab and not args.packed:
        p.error("--packed_vocab needs --packed")
    if args.moe_prefill != "loop" and not args.packed:
        p.error("--moe_prefill needs --packed")
    if args.gguf and args.quant_weights_path:
        p.error("--gguf and --quant_weights_path are mutually exclusive")
    if args.kl_against not in ("none", "model") and not (args.kl_against.startswith("gguf:") and args.kl_against[5:]):
        p.error("--kl_against must be none, model or gguf:FILE")
    for name in args.eval_datasets:  # refused BEFORE any work
        if not os.path.isfile(name):
            p.error(f"eval_datasets must be a .pt file of token-id tensors (got {name!r}); "
                    "dataset downloads are not part of this package")
    return args


_CONFIG_FILE = re.compile(r"\(([^()]+\.pth)\)\s*$")  # evo_quant_search's `<bitwidth> (<file name>)`


def load_compressed_weights(model, compressed_weights_path, compressed_config_path=None, default_level=0, load=None):
    """ppleval.py:124-152: with a config (lines `layer_name: level`, or `layer_name: bitwidth (file name)` as
    evo_quant_search writes them) exactly the listed layers get the weights of their level, without one every layer
    directory of the database gets `default_level`.  load(path, device) -> tensor
    (default torch.load onto the layer's device)."""
    if load is None:
        load = lambda path, device: torch.load(path, map_location=device)  # noqa: E731
    if compressed_config_path:
        with open(compressed_config_path) as f:
            todo = [tuple(x.strip() for x in line.split(":")) for line in f if line.strip()]
    else:
        todo = [(n, default_level) for n in sorted(os.listdir(compressed_weights_path))
                if os.path.isdir(os.path.join(compressed_weights_path, n))]
    for layer_name, level in todo:
        layer = model.get_submodule(layer_name)
        named = _CONFIG_FILE.search(str(level))  # the search's own lines: `name: 4.5 (4.5-Q4_K.pth)` names the file
        if named:
            path = os.path.join(compressed_weights_path, layer_name, named.group(1))
            if not os.path.isfile(path):
                raise FileNotFoundError(f"{path}: the weight file named by the configuration line of {layer_name}")
        else:
            path = level_db.find_level_file(os.path.join(compressed_weights_path, layer_name), level)
        w = load(path, layer.weight.device)
        if tuple(w.shape) != tuple(layer.weight.shape):
            raise ValueError(f"{layer_name}: level {level!r} has shape {tuple(w.shape)}, the model expects "
                             f"{tuple(layer.weight.shape)}")
        layer.weight.data = w.to(layer.weight.dtype)
    return model


def load_hf_model(args, device):
    import transformers
    from transformers import AutoModelForCausalLM
    dtype = args.dtype if args.dtype == "auto" else getattr(torch, args.dtype)
    dtype_kw = "dtype" if int(transformers.__version__.split(".")[0]) >= 5 else "torch_dtype"  # renamed in 5.x
    model = AutoModelForCausalLM.from_pretrained(args.model_name_or_path, low_cpu_mem_usage=True,
                                                 attn_implementation=args.attn_implementation, **{dtype_kw: dtype})
    model.config.use_cache = False
    return model.to(device).eval()


def apply_weights(model, args):
    """The scored model: --gguf, the level database, or the HF weights as loaded."""
    if args.gguf:
        packed = getattr(args, "packed", False)
        prefill = getattr(args, "moe_prefill", "loop")  # (named only where it is not the loader's default)
        gguf_loader.load_into_model(model, args.gguf, packed="all" if packed and getattr(args, "packed_vocab", False) else packed,
                                    **({"moe_prefill": prefill} if prefill != "loop" else {}))
    elif args.quant_weights_path:
        load_compressed_weights(model, args.quant_weights_path, args.quant_config_path, args.quant_default_level)
    return model


def main(argv=None):
    args = parse_args(argv)
    assert torch.cuda.is_available(), "ppleval needs a GPU (there is no CPU path)"
    device = torch.device("cuda")
    metrics.fix_seed(args.seed)
    model = load_hf_model(args, device)
    args.sequence_length = args.sequence_length or model.config.max_position_embeddings
    datasets = [metrics.load_eval_data(n, args.eval_tokens, args.sequence_length) for n in args.eval_datasets]

    targets = None
    if args.kl_against != "none":  # the target first: its logits stay on the device, then the scored weights are loaded
        if args.kl_against.startswith("gguf:"):
            gguf_loader.load_into_model(model, args.kl_against[5:])
        targets = [metrics.collect_target_logits(model, d) for d in datasets]
        if args.kl_against.startswith("gguf:"):  # back to the HF weights a level database is laid over
            model = load_hf_model(args, device)
    apply_weights(model, args)

    results = {
        "model_name_or_path": args.model_name_or_path,
        "evaluation_config": {"sequence_length": args.sequence_length, "eval_datasets": args.eval_datasets,
                              "eval_batch_size": args.eval_batch_size, "eval_tokens": args.eval_tokens, "seed": args.seed,
                              "dtype": str(args.dtype if args.dtype == "auto" else getattr(torch, args.dtype)),
                              "attn_implementation": args.attn_implementation},
        "compression_config": {"quant_weights_path": args.quant_weights_path, "quant_config_path": args.quant_config_path,
                               "quant_default_level": args.quant_default_level, "gguf": args.gguf},
        "perplexity_results": {},
    }
    print("-" * 10)
    print("Test perplexities")
    for name, data in zip(args.eval_datasets, datasets):
        ppl = metrics.compute_perplexity(model, data, batch_size=args.eval_batch_size)
        print(f"{name}: {ppl:.2f}")
        results["perplexity_results"][name] = float(ppl)
    if targets is not None:
        results["evaluation_config"]["kl_against"] = args.kl_against
        results["kl_results"] = {}
        print(f"KL divergence against {args.kl_against}")
        for name, data, tl in zip(args.eval_datasets, datasets, targets):
            kl = metrics.compute_kl_div(model, data, tl, batch_size=args.eval_batch_size)
            print(f"{name}: {kl:.6f}")
            results["kl_results"][name] = float(kl)
    print("-" * 10)
    with open(args.output_file, "w") as f:
        json.dump(results, f, indent=2)
    print(f"Results saved to {args.output_file}")
    return results


if __name__ == "__main__":
    main()
