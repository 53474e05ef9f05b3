#!/usr/bin/env python3
"""Let a model continue a prompt, greedily or by sampling: one prefill forward, then one-token forwards on the HF KV cache.
With `--gguf FILE --packed` the Linears of the blocks stay GGUF block bytes on the device and every decode step reads them
through gq_gemv_packed (PackedLinear routes inputs of a few tokens there), the prefill through gq_linear_packed; with
`--packed_vocab` token_embd and output stay packed as well.  With `--do_sample` every new token is one gq_sample_logits
launch on the last row of logits (temperature, top-k, top-p, the draw) and a row stops at `--eos_token_id`.

    python -m gptq_gguf_toolkit_amd.generate --model_name_or_path HF_DIR --prompt_ids ids.pt --max_new_tokens N \
        --output_file out.json [--gguf FILE [--packed [--moe_prefill grouped]] | --quant_weights_path DB --quant_config_path CFG] \
        [--dtype float16] [--attn_implementation eager] [--tokenizer_name NAME]

Prompts are the `.pt` list of [1, L] id tensors that ppleval reads (no tokenizer is needed; with --tokenizer_name the new
ids are also decoded to text).  The model is built by ppleval.load_hf_model / apply_weights.  Not here: an unbounded nucleus
(--top_k 0), min-p and repetition penalties, beam search, a generation config, graph capture of the decode step."""
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

from . import ops, ppleval  # noqa: E402


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


@torch.no_grad()
def sample(model, input_ids, max_new_tokens, temperature=1.0, top_k=40, top_p=1.0, generator=None, eos_token_id=None,
           pad_token_id=None, eos_poll=8, return_logits=False, timings=None):
    """input_ids [B, L] -> ids [B, L + M], 1 <= M <= max_new_tokens: a sampled continuation.  One forward over the prompt that
    keeps the last position's logits only (logits_to_keep=1: a packed lm_head never produces [L, V]), then one-token forwards
    on the cache.  Every new token is ops.sample_logits of the last row -- temperature, then top_k, then top_p, then the
    inverse CDF at u = torch.rand(B, generator=generator) on the model's device; temperature == 0 is the argmax with the lowest
    index among equals and draws nothing.  1 <= top_k <= ops.SAMPLE_MAX_K: there is no unbounded nucleus.
    eos_token_id (an int or a list): a row that has produced one is finished; from then on it is fed and filled with
    pad_token_id (default: the first eos id) and its draws are ignored.  The finished mask lives on the device; the host asks
    `finished.all()` once every eos_poll steps and makes no other synchronise per step; the result is cut after the last step
    in which any row was unfinished, so M does not depend on eos_poll.  With return_logits also the [B, M, V] logits the
    tokens were drawn from.  `timings` receives prefill_s, decode_s (as greedy) and stopped_at_eos (every row finished)."""
    if input_ids.dim() != 2 or input_ids.shape[1] < 1 or max_new_tokens < 1:
        raise ValueError(f"sample: input_ids must be [B, L >= 1] and max_new_tokens >= 1; got {tuple(input_ids.shape)}, "
                         f"{max_new_tokens}")
    if not 1 <= int(top_k) <= ops.SAMPLE_MAX_K:
        raise ValueError(f"sample: top_k={top_k} (not in [1, {ops.SAMPLE_MAX_K}]; an unbounded nucleus is not built)")
    if not 0 < top_p <= 1 or not temperature >= 0 or eos_poll < 1:
        raise ValueError(f"sample: top_p={top_p} must be in (0, 1], temperature={temperature} >= 0, eos_poll={eos_poll} >= 1")
    eos = [] if eos_token_id is None else [int(e) for e in (eos_token_id if isinstance(eos_token_id, (list, tuple))
                                                            else [eos_token_id])]
    B, dev = input_ids.shape[0], input_ids.device
    sync = torch.cuda.synchronize if input_ids.is_cuda else (lambda: None)
    if eos:
        eos_t = torch.tensor(eos, dtype=torch.int64, device=dev)
        pad = int(eos[0] if pad_token_id is None else pad_token_id)
        finished = torch.zeros(B, dtype=torch.bool, device=dev)
    rows, new, alive = [], [], []  # alive[i]: a 0-d bool on the device, "some row was unfinished when step i drew"

    def draw(logits):
        nonlocal finished
        row = logits[:, -1]
        u = None if temperature == 0 else torch.rand(B, generator=generator, device=dev)
        tok = ops.sample_logits(row, u, top_k, top_p, temperature)
        if eos:
            alive.append(~finished.all())
            tok = torch.where(finished, pad, tok)
            finished = finished | torch.isin(tok, eos_t)
        rows.append(row)
        new.append(tok)

    sync()
    t0 = time.perf_counter()
    out = model(input_ids=input_ids, use_cache=True, logits_to_keep=1)
    draw(out.logits)
    sync()
    t1 = time.perf_counter()
    stopped = False
    for step in range(1, max_new_tokens):
        if eos and step % eos_poll == 0 and bool(finished.all()):
            stopped = True
            break
        out = model(input_ids=new[-1][:, None], past_key_values=out.past_key_values, use_cache=True)
        draw(out.logits)
    sync()
    t2 = time.perf_counter()
    M = len(new)
    if eos:
        stopped = bool(finished.all())
        M = max(1, int(torch.stack(alive).sum()))  # (alive is a prefix of ones: a finished row stays finished)
    if timings is not None:
        timings.update(prefill_s=t1 - t0, decode_s=t2 - t1, stopped_at_eos=stopped)
    ids = torch.cat([input_ids, torch.stack(new[:M], 1)], 1)
    return (ids, torch.stack(rows[:M], 1)) if return_logits else ids


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--model_name_or_path", type=str, required=True, help="The name or path of the HF model (config, and the "
                                                                          "weights --gguf / the database do not replace)")
    p.add_argument("--prompt_ids", type=str, required=True, help=".pt file: a list of [1, L] token-id tensors, one per prompt")
    p.add_argument("--max_new_tokens", type=int, required=True, help="Tokens to generate per prompt")
    p.add_argument("--output_file", type=str, required=True, help="Path to the output JSON file")
    p.add_argument("--gguf", type=str, default=None, help="take ALL weights from this .gguf (decoded on the GPU)")
    p.add_argument("--packed", default=False, action="store_true",
                   help="with --gguf: keep the K-quant / Q8_0 / IQ4_NL / IQ4_XS weights of the blocks' Linears packed on the device")
    p.add_argument("--packed_vocab", default=False, action="store_true",
                   help="with --packed: keep token_embd and output packed as well (a PackedEmbedding and a packed lm_head)")
    p.add_argument("--moe_prefill", type=str, default="loop", choices=["loop", "grouped"],
                   help="with --packed: the prompt of a MoE model through the per-expert loop, or through device-side routing "
                        "and one grouped GEMM per projection")
    p.add_argument("--do_sample", default=False, action="store_true", help="sample (gq_sample_logits) instead of the argmax")
    p.add_argument("--temperature", type=float, default=1.0, help="with --do_sample: 0 is the argmax")
    p.add_argument("--top_k", type=int, default=40, help=f"with --do_sample: 1 .. {ops.SAMPLE_MAX_K} (there is no 'off')")
    p.add_argument("--top_p", type=float, default=1.0, help="with --do_sample: the nucleus mass, in (0, 1]")
    p.add_argument("--seed", type=int, default=0, help="with --do_sample: seed of the device generator of the draws")
    p.add_argument("--eos_token_id", type=int, nargs="+", default=None, help="with --do_sample: a prompt stops at these ids")
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
    if args.packed_vocab and not args.packed:
        p.error("--packed_vocab needs --packed")
    if args.moe_prefill != "loop" and not args.packed:
        p.error("--moe_prefill needs --packed")
    if not 1 <= args.top_k <= ops.SAMPLE_MAX_K:
        p.error(f"--top_k must be in [1, {ops.SAMPLE_MAX_K}] (an unbounded nucleus is not built)")
    if not 0 < args.top_p <= 1 or not args.temperature >= 0:
        p.error("--top_p must be in (0, 1] and --temperature >= 0")
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
    generator = None
    if args.do_sample:
        generator = torch.Generator(device=device)
        generator.manual_seed(args.seed)
    for ids in prompts:
        tm = {}
        if args.do_sample:
            out = sample(model, ids.to(device), args.max_new_tokens, args.temperature, args.top_k, args.top_p, generator,
                         args.eos_token_id, timings=tm)
        else:
            out = greedy(model, ids.to(device), args.max_new_tokens, timings=tm)
        new = out[0, ids.shape[1]:].tolist()
        steps = len(new) - 1  # the first new token comes from the prefill
        rec = {"prompt_tokens": int(ids.shape[1]), "new_ids": new, "prefill_s": tm["prefill_s"], "decode_s": tm["decode_s"],
               "decode_tokens_per_s": steps / tm["decode_s"] if steps and tm["decode_s"] > 0 else None}
        if args.do_sample:
            rec.update(sampled=True, seed=args.seed, stopped_at_eos=tm["stopped_at_eos"])
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
