#!/usr/bin/env python3
"""HF-named level configuration -> GGUF-named one: the reference's mapper/config_converter.py.

The search writes `model.layers.3.self_attn.q_proj: 4.5 (4.5-Q4_K.pth)` per Linear (evo_quant_search.configuration_text); the
stitcher wants `blk.3.attn_q.weight: 4.5 (4.5-Q4_K.pth)`.  Same functions, CLI and output text as the reference, pinned to
the reference's own run by tests/golden/G20_config_convert.json:

    python -m gptq_gguf_toolkit_amd.config_converter evo-kl-configuration-4.0.txt -o gguf_config.txt [--missing-value V]
        [--moe | --dense] [-v]

Rules (reference :27-136): everything after a line's first ':' is the value, verbatim; per block every component of the
dense or MoE table is written, from the input or as `missing_value`; attn_norm / ffn_norm always get `missing_value`; the
MoE table's q / k norms get it unless the input set them; outside the blocks embed_tokens / lm_head / model.norm are
renamed and any other key is kept as it is."""
import argparse
import sys
from pathlib import Path
from typing import Dict

# HF component of a decoder block -> GGUF tensor suffix, in the order the reference walks them (:42-71)
DENSE_COMPONENTS = (("mlp.down_proj", "ffn_down.weight"), ("mlp.gate_proj", "ffn_gate.weight"), ("mlp.up_proj", "ffn_up.weight"),
                    ("self_attn.k_proj", "attn_k.weight"), ("self_attn.q_proj", "attn_q.weight"),
                    ("self_attn.v_proj", "attn_v.weight"), ("self_attn.o_proj", "attn_output.weight"))
MOE_COMPONENTS = (("self_attn.k_proj", "attn_k.weight"), ("self_attn.q_proj", "attn_q.weight"),
                  ("self_attn.v_proj", "attn_v.weight"), ("self_attn.o_proj", "attn_output.weight"),
                  ("mlp.experts.down_proj", "ffn_down_exps.weight"), ("mlp.experts.gate_proj", "ffn_gate_exps.weight"),
                  ("mlp.experts.up_proj", "ffn_up_exps.weight"), ("mlp.gate", "ffn_gate_inp.weight"),
                  ("self_attn.k_norm", "attn_k_norm.weight"), ("self_attn.q_norm", "attn_q_norm.weight"))
# substring of a key outside the blocks -> GGUF tensor, first match wins (:124-129)
TOP_LEVEL = (("embed_tokens", "token_embd.weight"), ("lm_head", "output.weight"), ("model.norm", "output_norm.weight"))
MOE_INDICATORS = ("experts", "mlp.gate.", "router", "shared_expert")  # :162-167
BLOCK_MARK = "model.layers."


def _parse(hf_config: str) -> Dict[str, str]:
    """{key: value} of the `key: value` lines; blank lines, '#' lines and lines without ':' are dropped; a repeated key
    keeps its first position and its last value (a dict)."""
    pairs = {}
    for line in hf_config.strip().split("\n"):
        line = line.strip()
        if not line or line.startswith("#") or ":" not in line:
            continue
        key, value = line.split(":", 1)
        pairs[key.strip()] = value.strip()
    return pairs


def convert_hf_to_gguf_config(hf_config: str, missing_value: str = "32", is_moe: bool = False) -> Dict[str, str]:
    pairs = _parse(hf_config)
    components = MOE_COMPONENTS if is_moe else DENSE_COMPONENTS
    blocks: Dict[int, Dict[str, str]] = {}
    for key, value in pairs.items():
        if BLOCK_MARK not in key:
            continue
        parts = key.split(".")  # model.layers.<n>.<component...>: the block number is the THIRD field (:77-87)
        if len(parts) < 4:
            continue
        try:
            number = int(parts[2])
        except ValueError:
            continue
        blocks.setdefault(number, {})[".".join(parts[3:])] = value
    out: Dict[str, str] = {}
    for number in sorted(blocks):
        given = blocks[number]
        for present in (True, False):  # the components the input names first, then the missing ones (:100-107)
            for hf, gg in components:
                if (hf in given) == present:
                    out[f"blk.{number}.{gg}"] = given[hf] if present else missing_value
        out[f"blk.{number}.attn_norm.weight"] = missing_value
        out[f"blk.{number}.ffn_norm.weight"] = missing_value
        if is_moe:  # both are in the MoE table already, so this never changes a value (:113-118)
            out.setdefault(f"blk.{number}.attn_k_norm.weight", missing_value)
            out.setdefault(f"blk.{number}.attn_q_norm.weight", missing_value)
    for key, value in pairs.items():
        if BLOCK_MARK in key:
            continue
        out[next((gg for mark, gg in TOP_LEVEL if mark in key), key)] = value
    return out


def read_config_file(filepath: str) -> str:
    with open(filepath, "r") as f:
        return f.read()


def config_text(config_dict: Dict[str, str]) -> str:
    return "".join(f"{key}: {config_dict[key]}\n" for key in sorted(config_dict))


def write_config_file(config_dict: Dict[str, str], filepath: str) -> None:
    with open(filepath, "w") as f:
        f.write(config_text(config_dict))


def detect_moe_model(hf_config: str) -> bool:
    """A line that mentions experts, a router or `mlp.gate.` makes the model MoE (case-insensitive, :162-174)."""
    return any(mark in line.strip().lower() for line in hf_config.strip().split("\n") for mark in MOE_INDICATORS)


def main(argv=None):
    p = argparse.ArgumentParser(description="Convert HuggingFace model layer configuration to GGUF format")
    p.add_argument("input_file", type=str, help="Path to the HuggingFace configuration file")
    p.add_argument("-o", "--output", type=str, help="Output file path (default: print to stdout)")
    p.add_argument("--missing-value", type=str, default="32 (32-F32.pth)",
                   help='Value to use for missing layers (default: "32 (32-F32.pth)")')
    p.add_argument("--moe", action="store_true", help="Force MoE model mode")
    p.add_argument("--dense", action="store_true", help="Force dense model mode")
    p.add_argument("-v", "--verbose", action="store_true", help="Enable verbose output")
    args = p.parse_args(argv)

    def fail(message):
        print(f"Error: {message}", file=sys.stderr)
        sys.exit(1)

    path = Path(args.input_file)
    if not path.exists():
        fail(f"Input file '{args.input_file}' does not exist.")
    if not path.is_file():
        fail(f"'{args.input_file}' is not a file.")
    if args.moe and args.dense:
        fail("Cannot specify both --moe and --dense flags.")
    try:
        hf_config = read_config_file(args.input_file)
        is_moe = True if args.moe else False if args.dense else detect_moe_model(hf_config)
        if args.verbose:
            print(f"Reading HuggingFace config from: {args.input_file}")
            print(f"Model type detected: {'MoE' if is_moe else 'Dense'}")
            print(f"Using '{args.missing_value}' for missing values")
        gguf_config = convert_hf_to_gguf_config(hf_config, args.missing_value, is_moe)
        if args.verbose:
            print(f"Converted {len(gguf_config)} layer configurations")
        if args.output:
            write_config_file(gguf_config, args.output)
            if args.verbose:
                print(f"GGUF config written to: {args.output}")
        else:
            sys.stdout.write(config_text(gguf_config))
    except Exception as e:  # the reference reports and exits 1
        fail(e)


if __name__ == "__main__":
    main()
