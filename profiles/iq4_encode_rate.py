"""The IQ4_NL / IQ4_XS encoder (gq_quantize_iq4): kernel figures and where the level lands, one JSON line per part.  One process,
HIP events around each launch, warm-up first, the candidates ALTERNATING (every candidate takes every place in the order), median
of N with min-max.
  encode  gq_quantize_iq4 on bf16 input at [4096, 4096], [14336, 4096] and [4096, 14336]: IQ4_XS and IQ4_NL, with and without
          importance, beside gq_quantize_q8_0 (the parent commit's encoder) on the same tensor, and beside the time the call's
          bytes -- every input read once, every output written once -- take at the device's HBM rate
  build   the one-pass level build of the tests' tiny Llama (levels Q3_K and Q4_K into a level database) with and without
          level_db_iq4=("IQ4_XS", "IQ4_NL"): host wall time of Quantizer.quantize_levels, the two alternating
  rung    ErrorEstimator on that database: the summed layer error of the Hessian-weighted IQ4_XS level, of the unweighted one
          (level_db_iq4_importance="none") and of the Q3_K / Q4_K GPTQ levels.  A record, asserted nowhere.
usage: python profiles/iq4_encode_rate.py [N=15] [--work DIR]   (GPU box; needs the built tree and tests/golden)"""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402
from gptq_gguf_toolkit_amd import ops  # noqa: E402

HBM_PEAK = 8.0e12
XS, NL = 23, 20
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(argv[0]) if argv and argv[0].isdecimal() else 15
LINEARS = r".*layers.*((q|k|v|o|gate|up|down)_proj)$"


def flag(name):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None


def measure(cands):
    for fn in cands.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times, keys = {k: [] for k in cands}, list(cands)
    for it in range(N):
        evs = []
        for k in keys[it % len(keys):] + keys[:it % len(keys)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cands[k]()
            e1.record()
            evs.append((k, e0, e1))
        torch.cuda.synchronize()
        for k, e0, e1 in evs:
            times[k].append(e0.elapsed_time(e1) * 1e-3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def encode():
    for R, C in ((4096, 4096), (14336, 4096), (4096, 14336)):
        torch.manual_seed(0)
        x = (torch.randn(R, C, device="cuda") * 0.02).bfloat16()
        imp = torch.rand(C, device="cuda") ** 4 * 10 + 1e-3
        out_bytes = {"xs": R * C // 256 * 136, "nl": R * C // 32 * 18, "q8_0": R * C // 32 * 34}
        m = measure({"xs": lambda: ops.quantize_iq4(x, XS), "xs_importance": lambda: ops.quantize_iq4(x, XS, imp),
                     "nl": lambda: ops.quantize_iq4(x, NL), "nl_importance": lambda: ops.quantize_iq4(x, NL, imp),
                     "q8_0": lambda: ops.quantize_q8_0(x)})
        row = {"part": "encode_from_bf16", "launches": N, "R": R, "C": C, "hbm_peak_TBps": HBM_PEAK / 1e12}
        for k, (med, lo, hi) in m.items():
            nbytes = 2 * R * C + out_bytes[k.split("_imp")[0]] + (4 * C if "importance" in k else 0)
            row[k] = {"us": round(med * 1e6, 1), "min_us": round(lo * 1e6, 1), "max_us": round(hi * 1e6, 1),
                      "bytes_per_param": round(nbytes / (R * C), 4), "us_at_hbm_peak": round(nbytes / HBM_PEAK * 1e6, 1),
                      "Gparam_per_s": round(R * C / med / 1e9, 1), "over_q8_0": round(med / m["q8_0"][0], 1)}
        print(json.dumps(row), flush=True)
        del x


def drive(work, tag, levels, **kw):
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    from gptq_gguf_toolkit_amd.quantizer import Quantizer
    model = tiny_llama()
    model_dir = os.path.join(work, "model")
    if not os.path.isdir(model_dir):
        model.save_pretrained(model_dir)
    model = model.cuda()
    data = [([], {"input_ids": ids}) for ids in tiny_calib()]
    drv = Quantizer(model, data_loader=data, quantizable_modules=LINEARS,
                    quantizer_kwargs=dict(rel_damp=0.01, block_size=128, act_order=False, quant_scale="absmax",
                                          static_groups=False, rmin=-1.0, rdelta=0.1, nstep=20, verbose=False),
                    pre_block_modules=["model.embed_tokens"], block_modules="model.layers", post_block_modules=["lm_head"],
                    quant_non_block_modules=False, device="cuda:0", save_dir=os.path.join(work, tag))
    db = os.path.join(work, f"db_{tag}")
    shutil.rmtree(db, ignore_errors=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    drv.quantize_levels([T[n] for n in levels], T[levels[-1]], level_db=db, level_db_model=model_dir, level_db_vocab=False,
                        trees=False, **kw)
    torch.cuda.synchronize()
    return db, time.perf_counter() - t0


def build_and_rung(work):
    from make_golden_shim import tiny_calib, tiny_llama
    from gptq_gguf_toolkit_amd.error_estimator import ErrorEstimator
    os.environ.setdefault("GQ_SAVE_SLOT_MB", "8")
    levels = ["Q3_K", "Q4_K"]
    drive(work, "warm", levels)  # the first build of a process pays the one-time costs
    times = {"plain": [], "iq4": []}
    for it in range(3):
        for k in (("plain", "iq4") if it % 2 == 0 else ("iq4", "plain")):
            kw = {"level_db_iq4": ("IQ4_XS", "IQ4_NL")} if k == "iq4" else {}
            times[k].append(drive(work, k, levels, **kw)[1])
    print(json.dumps({"part": "level_build_tiny_llama", "levels": levels, "builds_each": 3,
                      "plain_s": [round(t, 3) for t in times["plain"]], "with_iq4_xs_and_nl_s": [round(t, 3) for t in times["iq4"]],
                      "median_plain_s": round(statistics.median(times["plain"]), 3),
                      "median_with_iq4_s": round(statistics.median(times["iq4"]), 3)}), flush=True)
    row = {"part": "estimator_rung_tiny_llama", "what": "sum over the 14 Linears of ErrorEstimator's layer error, per level"}
    for tag, kw in (("weighted", {}), ("unweighted", {"level_db_iq4_importance": "none"})):
        db, _ = drive(work, f"rung_{tag}", levels, level_db_iq4=("IQ4_XS",), **kw)
        model = tiny_llama(dtype=torch.float16).cuda()
        data = [([], {"input_ids": ids}) for ids in tiny_calib()[:4]]
        est = ErrorEstimator(model, data, LINEARS, ["model.embed_tokens"], "model.layers", db, device="cuda:0")
        errors = est.estimate()[-1]
        total = {}
        for n, errs in errors.items():
            for f, e in zip(est.levels[n], errs):
                total[f[:-4]] = total.get(f[:-4], 0.0) + float(e)
        row[tag] = {k: float(f"{v:.4e}") for k, v in sorted(total.items())}
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    encode()
    work = flag("--work") or tempfile.mkdtemp(prefix="iq4_rate_")
    os.makedirs(work, exist_ok=True)
    build_and_rung(work)
