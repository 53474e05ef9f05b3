"""Wall time of a whole ErrorEstimator.estimate on the random-init Llama-3-8B of `bench.py --full`, two levels, one JSON line.
The model is built on the GPU in bf16 (no download); the level database is made here: RTN Q2_K and Q4_K of every decoder
Linear (ops.rtn_quantize + ops.dequantize), torch-saved in fp16 under a temporary directory.  The walk is timed on the host
around a final synchronize; inside it ops.h_accumulate and ops.quad_form are bracketed by HIP events (sum of launch
durations on the stream) and the level reads (torch.load onto the device) by the host clock; "forward" is the rest:
the block forwards, the hooks and the host logic.
--layers N walks a model of N blocks (default 2) and also reports the figure scaled to 32: a block's cost does not depend on its
index, and 32 blocks x 7 Linears x 2 levels are 98 GB of level files.
usage: python profiles/errest_wall.py [--layers 2] [--nseq 16] [--seq_len 2048]   (GPU box; needs only the built tree)"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from gptq_gguf_toolkit_amd import error_estimator as ee, level_db, ops  # noqa: E402

CFG = dict(hidden_size=4096, intermediate_size=14336, num_attention_heads=32, num_key_value_heads=8, vocab_size=128256,
           max_position_embeddings=8192, rope_theta=500000.0, rms_norm_eps=1e-5)
LEVELS = (("2-Q2_K.pth", 10), ("4-Q4_K.pth", 12))


def build_model(layers):
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(tie_word_embeddings=False, attn_implementation="sdpa", num_hidden_layers=layers, **CFG)
    torch.manual_seed(0)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device("cuda"):
            model = LlamaForCausalLM(cfg)
    finally:
        torch.set_default_dtype(old)
    return model.eval()


class Timed:
    """ops, with h_accumulate / quad_form bracketed by HIP events and the level reads by the host clock."""

    def __init__(self):
        self.ev = {"syrk": [], "quad_form": []}
        self.load_s = 0.0

    def _wrap(self, key, fn):
        def call(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            self.ev[key].append((e0, e1))
            return out
        return call

    def __getattr__(self, name):
        if name == "h_accumulate":
            return self._wrap("syrk", ops.h_accumulate)
        if name == "quad_form":
            return self._wrap("quad_form", ops.quad_form)
        return getattr(ops, name)

    def ms(self, key):
        return sum(a.elapsed_time(b) for a, b in self.ev[key])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--nseq", type=int, default=16)
    ap.add_argument("--seq_len", type=int, default=2048)
    a = ap.parse_args()
    model = build_model(a.layers)
    g = torch.Generator().manual_seed(1)
    data = [([], {"input_ids": torch.randint(0, CFG["vocab_size"], (1, a.seq_len), generator=g)}) for _ in range(a.nseq)]
    db = tempfile.mkdtemp(prefix="errest_levels_")
    try:
        names = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and ".layers." in n]
        for n in names:
            W = model.get_submodule(n).weight.detach().contiguous()
            os.makedirs(os.path.join(db, n))
            for f, qt in LEVELS:
                torch.save(ops.dequantize(qt, *ops.rtn_quantize(W, qt), out_dtype=torch.float16).cpu(), os.path.join(db, n, f))
        timed = Timed()
        ee._ops = timed
        inner = level_db.load_level

        def load_level(*x, **k):
            t0 = time.perf_counter()
            w = inner(*x, **k)
            torch.cuda.current_stream().synchronize()
            timed.load_s += time.perf_counter() - t0
            return w

        level_db.load_level = load_level
        est = ee.ErrorEstimator(model, data, r".*layers.*((q|k|v|o|gate|up|down)_proj)$", ["model.embed_tokens", "model.rotary_emb"],
                                "model.layers", db, device="cuda:0")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        errors = est.estimate()[-1]
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    finally:
        shutil.rmtree(db, ignore_errors=True)
    syrk, quad = timed.ms("syrk") / 1e3, timed.ms("quad_form") / 1e3
    rest = wall - syrk - quad - timed.load_s
    worst = max(v[0] for v in errors.values())
    print(json.dumps({
        "model": f"random-init Llama-3-8B shapes, {a.layers} blocks, bf16", "nseq": a.nseq, "seq_len": a.seq_len, "levels": len(LEVELS),
        "linears": len(names), "wall_s": round(wall, 3), "syrk_s": round(syrk, 3), "syrk_launches": len(timed.ev["syrk"]),
        "quad_form_s": round(quad, 3), "quad_form_calls": len(timed.ev["quad_form"]), "level_load_s": round(timed.load_s, 3),
        "forward_and_host_s": round(rest, 3), "wall_s_scaled_to_32_blocks": round(wall * 32 / a.layers, 1),
        "largest_q2k_error": worst}))


if __name__ == "__main__":
    main()
