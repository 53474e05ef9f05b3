#!/usr/bin/env python3
"""Let a model continue a prompt, greedily: one prefill forward, then one-token forwards on the HF KV cache.  With
`--gguf FILE --packed` the Linears of the blocks stay GGUF block bytes on the device and every decode step reads them through
gq_gemv_packed (PackedLinear routes inputs of a few tokens there), the prefill through gq_linear_packed.

    python -m gptq_gguf_toolkit_amd.generate --model_name_or_path HF_DIR --prompt_ids ids.pt --max_new_tokens N \
        --output_file out.json [--gguf FILE [--packed] | --quant_weights_path DB --quant_config_path CFG] \
        [--dtype float16] [--attn_implementation eager] [--tokenizer_name NAME]

Prompts are the `.pt` list of [1, L] id tensors that ppleval reads (no tokenizer is needed; with --tokenizer_name the new
ids are also decoded to text).  The model is built by ppleval.load_hf_model / apply_weights.  Not here: sampling, EOS
handling, a generation config, graph capture of the decode step."""
import argparse
import json
import os
import sys
import time

import torch

if __package__ in (None, ""):  # run as a script: make the package importable under its alias
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gptq_gguf_toolkit_amd  # noqa: F401
    __package__ = "gptq_gguf_toolkit_amd"

from . import ppleval  # noqa: E402


@torch.no_grad()
def greedy(model, input_ids, max_new_tokens, return_logits=False, timings=None):
    """input_ids [B, L] -> ids [B, L + N], N = max_new_tokens >= 1: the argmax continuation.  One forward over the prompt,
    then N - 1 forwards of one token each with the cache the previous forward returned.  With return_logits also the
    [B, N, V] logits each new token was the argmax of.  `timings`, a dict, receives prefill_s and decode_s (wall time up to a
    device synchronise after the prefill and after the last step)."""
    if input_ids.dim() != 2 or input_ids.shape[1] < 1 or max_new_tokens < 1:
        raise ValueError(f"greedy: input_ids must be [B, L >= 1] and max_new_tokens >= 1; got {tuple(input_ids.shape)}, "
                         f"{max_new_tokens}")
    sync = torch.cuda.synchronize if input_ids.is_cuda else (lambda: None)
    sync()
    t0 = time.perf_counter()
    out = model(input_ids=input_ids, use_cache=True)
    rows = [out.logits[:, -1]]
    new = [rows[-1].argmax(-1)]
    sync()
    t1 = time.perf_counter()
    for _ in range(max_new_tokens - 1):
        out = model(input_ids=new[-1][:, None], past_key_values=out.past_key_values, use_cache=True)
        rows.append(out.logits[:, -1])
        new.append(rows[-1].argmax(-1))
    sync()
    t2 = time.perf_counter()
    if timings is not None:
        timings.update(prefill_s=t1 - t0, decode_s=t2 - t1)
    ids = torch.cat([input_ids, torch.stack(new, 1)], 1)
    return (ids, torch.stack(rows, 1)) if return_logits else ids


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--model_name_or_path", type=str, required=True, help="The name or path of the HF model (config, and the "
                                                                          "weights --gguf / the database do not replace)")
    p.add_argument("--prompt_ids", type=str, required=True, help=".pt file: a list of [1, L] token-id tensors, one per prompt")
    p.add_argument("--max_new_tokens", type=int, required=True, help="Tokens to generate per prompt")
    p.add_argument("--output_file", type=str, required=True, help="Path to the output JSON file")
    p.add_argument("--gguf", type=str, default=None, help="take ALL weights from this .gguf (decoded on the GPU)")
    p.add_argument("--packed", default=False, action="store_true",
                   help="with --gguf: keep the K-quant / Q8_0 weights of the blocks' Linears packed on the device")
    p.add_argument("--quant_weights_path", type=str, default=None, help="Path to quantized weights (a level database)")
    p.add_argument("--quant_config_path", type=str, default=None, help="Path to quantization config")
    p.add_argument("--quant_default_level", type=int, default=0, help="Default quantization level")
    p.add_argument("--dtype", type=str, default="float16", choices=["auto", "float16", "float32", "bfloat16"],
                   help="dtype to load the model.")
    p.add_argument("--attn_implementation", type=str, default=None, choices=["eager", "sdpa", "flash_attention_2"],
                   help="Attention implementation: eager, sdpa, or flash_attention_2")
    p.add_argument("--tokenizer_name", type=str, default=None, help="also decode the new ids to text with this tokenizer")
    args = p.parse_args(argv)
    if args.packed and not args.gguf:
        p.error("--packed needs --gguf")
    if args.gguf and args.quant_weights_path:
        p.error("--gguf and --quant_weights_path are mutually exclusive")
    if args.quant_config_path and not args.quant_weights_path:
        p.error("--quant_config_path needs --quant_weights_path")
    if args.max_new_tokens < 1:
        p.error("--max_new_tokens must be at least 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    assert torch.cuda.is_available(), "generate needs a GPU (there is no CPU path)"
    device = torch.device("cuda")
    prompts = torch.load(args.prompt_ids)
    model = ppleval.apply_weights(ppleval.load_hf_model(args, device), args)
    tokenizer = None
    if args.tokenizer_name:
        from transformers import AutoTokenizer
        tokenizer = AutoTokenizer.from_pretrained(args.tokenizer_name)
    results = {"model_name_or_path": args.model_name_or_path, "gguf": args.gguf, "packed": args.packed,
               "quant_weights_path": args.quant_weights_path, "quant_config_path": args.quant_config_path,
               "max_new_tokens": args.max_new_tokens, "prompts": []}
    for ids in prompts:
        tm = {}
        out = greedy(model, ids.to(device), args.max_new_tokens, timings=tm)
        new = out[0, ids.shape[1]:].tolist()
        steps = args.max_new_tokens - 1  # the first new token comes from the prefill
        rec = {"prompt_tokens": int(ids.shape[1]), "new_ids": new, "prefill_s": tm["prefill_s"], "decode_s": tm["decode_s"],
               "decode_tokens_per_s": steps / tm["decode_s"] if steps and tm["decode_s"] > 0 else None}
        if tokenizer is not None:
            rec["text"] = tokenizer.decode(new)
        results["prompts"].append(rec)
        print(f"prompt of {rec['prompt_tokens']} tokens: prefill {rec['prefill_s'] * 1e3:.1f} ms, {steps} decode steps "
              f"{rec['decode_s'] * 1e3:.1f} ms")
    with open(args.output_file, "w") as f:
        json.dump(results, f, indent=2)
    print(f"Results saved to {args.output_file}")
    return results


if __name__ == "__main__":
    main()
