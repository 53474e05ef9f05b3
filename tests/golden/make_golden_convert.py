#!/usr/bin/env python3
"""G20: what the reference's configuration converter (read-only at /root/reference/mapper/config_converter.py, standard
library only) returns and writes for the inputs below, by IMPORTING AND CALLING it.  Recorded per case: the input text,
is_moe (None: the reference's own detect_moe_model decides, and its answer is recorded), missing_value, the returned dict
and the text write_config_file wrote -- tests/golden/G20_config_convert.json.  tests/test_stitch_cpu.py demands the same dict
and the same text of this package's config_converter.  Nothing of the reference is copied.  `python make_golden_convert.py`
runs only where the reference is; the tests read the fixture."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/mapper"
PROJ = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
        "mlp.down_proj")
LEVELS = ((2.5625, "Q2_K"), (4.5, "Q4_K"), (6.5625, "Q6_K"))


def search_result(blocks=2, numbers_only=False, drop=()):
    """The text evo_quant_search.configuration_text writes: `name: bw (bw-TYPE.pth)`, no trailing newline."""
    lines = []
    for b in range(blocks):
        for i, p in enumerate(PROJ):
            if (b, p) in drop:
                continue
            bw, t = LEVELS[(3 * b + i) % 3]
            lines.append(f"model.layers.{b}.{p}: {bw}" + ("" if numbers_only else f" ({bw}-{t}.pth)"))
    return "\n".join(lines)


def cases():
    """name -> (input text, is_moe or None for auto-detection, missing_value)"""
    commented = ("# evo search, generation 12\n\nmodel.layers.0.self_attn.q_proj: 4.5 (4.5-Q4_K.pth)\n"
                 "   # indented comment\nno colon on this line\n\n  model.layers.0.mlp.up_proj :  6.5625 Q6_K  \n"
                 "model.layers.1.self_attn.k_proj: a: b (c)\nmodel.layers.x.mlp.up_proj: 4\nmodel.layers.7: 3\n")
    mixtral = "\n".join(
        [f"model.layers.{b}.self_attn.{p}_proj: 4.5 (4.5-Q4_K.pth)" for b in range(2) for p in "qkvo"]
        + [f"model.layers.{b}.mlp.experts.{p}_proj: 2.5625 (2.5625-Q2_K.pth)" for b in range(2) for p in ("gate", "up")]
        + ["model.layers.0.mlp.experts.down_proj: 6.5625 (6.5625-Q6_K.pth)", "model.layers.0.mlp.gate: 16 (16-F16.pth)",
           "model.layers.1.self_attn.q_norm: 32 (32-F32.pth)",
           "model.layers.1.block_sparse_moe.experts.3.w1: 4.5 (4.5-Q4_K.pth)", "model.layers.1.mlp.down_proj: 4.5"])
    top = ("model.embed_tokens: 6.5625 (6.5625-Q6_K.pth)\nlm_head: 8.5 Q8_0\nmodel.norm: 32\nrope_freqs.weight: 32 F32\n"
           "model.layers.0.mlp.down_proj: 4.5 (4.5-Q4_K.pth)")
    return {
        "search_result": (search_result(), False, "32"),
        "search_result_cli_default": (search_result(), None, "32 (32-F32.pth)"),
        "plain_numbers": (search_result(numbers_only=True), False, "32"),
        "two_projections_missing": (search_result(drop={(1, "self_attn.v_proj"), (1, "mlp.down_proj")}), False,
                                    "16 (16-F16.pth)"),
        "comments_and_blanks": (commented, False, "32"),
        "mixtral": (mixtral, True, "32 (32-F32.pth)"),
        "mixtral_detected": (mixtral, None, "32"),
        "mixtral_read_as_dense": (mixtral, False, "32"),
        "top_level_and_unknown": (top, False, "32"),
    }


def main():
    sys.path.insert(0, REF)
    import config_converter as R
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (text, is_moe, missing) in cases().items():
            detected = R.detect_moe_model(text)
            d = R.convert_hf_to_gguf_config(text, missing, detected if is_moe is None else is_moe)
            path = os.path.join(tmp, name + ".txt")
            R.write_config_file(d, path)
            with open(path) as f:
                written = f.read()
            out[name] = {"input": text, "is_moe": is_moe, "detected_moe": detected, "missing_value": missing, "dict": d,
                         "keys_in_order": list(d), "written": written}
            print(name, len(d), "keys,", len(written), "bytes")
    with open(os.path.join(HERE, "G20_config_convert.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
