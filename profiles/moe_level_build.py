#!/usr/bin/env python3
"""One Mixtral-8x7B-shaped block (E = 8, H = 4096, I = 14336, 32 heads / 8 KV heads, bf16, random weights) through the
one-pass level build -- Quantizer.quantize_levels(5 K-quant levels, propagate Q4_K, fused_experts=True, level_db=DIR,
trees=False): one calibration, one Hessian and factorisation per input, one walk for all levels, the bands packed into
the stacked unit buffers -- against five single-level Quantizer.quantize() calls on the same block and calibration data
(each writes its tree, what the packer + splitter route starts from).  Wall time of each call, synchronised, files on
disk; peak device memory of each call from torch.cuda.memory_stats; the saver's own figures.  One unmeasured warm-up
call (Q4_K) first; clocks as found.

    python profiles/moe_level_build.py [OUT.txt]      (default: stdout only)"""
import os
import shutil
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T  # noqa: E402
from gptq_gguf_toolkit_amd.quantizer import Quantizer  # noqa: E402

E, H, I, HEADS, KV, V = 8, 4096, 14336, 32, 8, 512
SEQS, L = 4, 1024
LEVELS = ("Q2_K", "Q3_K", "Q4_K", "Q5_K", "Q6_K")
REGEX = r".*layers.*((q|k|v|o)_proj|experts\.\d+\.w[123])$"
KEYS = ("q_proj", "k_proj", "v_proj", "o_proj", "w1", "w2", "w3")
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


def quantizer(model, data, save_dir):
    return Quantizer(model, data_loader=data, quantizable_modules=REGEX,
                     quantizer_kwargs=dict(rel_damp=0.01, block_size=128, act_order=False, quant_scale="absmax",
                                           static_groups=False, rmin=-1.0, rdelta=0.1, nstep=20, verbose=False),
                     pre_block_modules=["model.embed_tokens"], block_modules="model.layers", post_block_modules=["lm_head"],
                     quant_non_block_modules=False, device="cuda:0", save_dir=save_dir)


def measured(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ms = torch.cuda.memory_stats()
    return dt, ms["allocated_bytes.all.peak"] / 2**30, ms["reserved_bytes.all.peak"] / 2**30


def du(path):
    return sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(path) for f in fs)


def main():
    from transformers import MixtralConfig, MixtralForCausalLM
    torch.manual_seed(0)
    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_hidden_layers=1, num_attention_heads=HEADS, num_key_value_heads=KV,
                        num_local_experts=E, num_experts_per_tok=2, vocab_size=V, max_position_embeddings=L,
                        tie_word_embeddings=False, router_jitter_noise=0.0)
    with torch.device("cuda"):
        model = MixtralForCausalLM(cfg).to(torch.bfloat16).eval()
    root = tempfile.mkdtemp(prefix="moe_level_build_")
    try:
        hf = os.path.join(root, "hf")
        model.save_pretrained(hf, safe_serialization=True)
        original = {k: v.detach().clone() for k, v in model.state_dict().items()}
        g = torch.Generator().manual_seed(3)
        data = [([], {"input_ids": torch.randint(0, V, (1, L), generator=g)}) for _ in range(SEQS)]
        base = torch.cuda.memory_allocated() / 2**30
        say(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; one block E={E} H={H} I={I} bf16, {SEQS} x {L} calibration "
            f"tokens; model + its copy resident: {base:.2f} GiB; GQ_SAVE_SLOT_MB={os.environ.get('GQ_SAVE_SLOT_MB', 'default')}")

        def single(name, tag):
            model.load_state_dict(original)
            d = os.path.join(root, tag)
            shutil.rmtree(d, ignore_errors=True)
            os.makedirs(d)
            q = quantizer(model, data, d)
            out = measured(lambda: q.quantize({k: T[name] for k in KEYS}))
            return out + (du(d), q)

        single("Q4_K", "warm")
        say("warm-up quantize(Q4_K) done (not measured)")
        total = 0.0
        for name in LEVELS:
            dt, alloc, resv, nbytes, q = single(name, "tree")
            total += dt
            say(f"quantize({name}):            {dt:8.2f} s   peak allocated {alloc:6.2f} GiB  reserved {resv:6.2f} GiB   tree {nbytes / 2**30:5.2f} GiB")
        say(f"five single-level calls:     {total:8.2f} s")

        model.load_state_dict(original)
        d = os.path.join(root, "levels")
        os.makedirs(d)
        q = quantizer(model, data, d)
        db = os.path.join(root, "db")
        dt, alloc, resv = measured(lambda: q.quantize_levels([T[n] for n in LEVELS], T.Q4_K, fused_experts=True, level_db=db,
                                                             level_db_model=hf, level_db_vocab=False, trees=False))
        say(f"quantize_levels(5 levels):   {dt:8.2f} s   peak allocated {alloc:6.2f} GiB  reserved {resv:6.2f} GiB   database "
            f"{du(db) / 2**30:5.2f} GiB")
        say(f"five calls / one pass:       {total / dt:8.2f} x")
        t = q.timing
        say(f"one pass, host seconds per phase: {t['host_s']}")
        say(f"one pass, saver: copy thread busy {t.get('saver_copy_thread_busy_s')} s, writer process busy "
            f"{t.get('saver_writer_process_busy_s')} s, close {t.get('saver_close_split_s')}")
        unit = max(os.path.getsize(os.path.join(db, n, f)) for n in os.listdir(db) if n.endswith("_exps.weight")
                   for f in os.listdir(os.path.join(db, n)) if f.endswith(".pth"))
        say(f"largest unit level file: {unit / 2**20:.0f} MiB; the block's packed expert bytes: "
            f"{sum(du(os.path.join(db, n)) for n in os.listdir(db) if n.endswith('_exps.weight')) / 2**30:.2f} GiB")
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
