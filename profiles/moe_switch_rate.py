"""The level switch of a stacked expert tensor, one JSON line per measurement: ONE job of gq_level_switch_experts against the E
per-expert jobs of gq_level_switch, same process, same source and destination buffers, at
  Mixtral-8x7B's  [8, 14336, 4096]   Q4_K and Q6_K -> bf16
  a many-expert   [128, 768, 2048]   Q4_K and Q6_K -> bf16
device_us  HIP events around one call of the library with a job table made beforehand;
host_us    the wall time of that call on the host (it only enqueues), table made beforehand;
ops_us     the wall time of the call through the Python binding (ops.level_switch_experts / ops.level_switch), which builds the
           table -- what LevelStore.switch pays per changed unit.
3 warm-up calls, median of 15 with min-max, the two forms alternating, clocks as found.  The two results are compared bit for
bit first.
usage: python profiles/moe_switch_rate.py [--out FILE]   (GPU box; needs only the built tree).  Writes FILE (default
profiles/moe_switch_rate.txt) and prints the same lines."""
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402
from gptq_gguf_toolkit_amd import _cabi, ops  # noqa: E402

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "moe_switch_rate.txt")
WARM, N = 3, 15
CASES = (("mixtral", 8, 14336, 4096), ("many-expert", 128, 768, 2048))
TYPES = (("Q4_K", 12), ("Q6_K", 14))


def stats(v):
    return {"us": round(statistics.median(v) * 1e6, 1), "min_us": round(min(v) * 1e6, 1), "max_us": round(max(v) * 1e6, 1)}


def measure(cands):
    """{name: call} -> {name: (device seconds, host seconds) lists}: events around the call, perf_counter around it too."""
    keys = list(cands)
    for k in keys:
        for _ in range(WARM):
            cands[k]()
    torch.cuda.synchronize()
    dev, host = {k: [] for k in keys}, {k: [] for k in keys}
    for it in range(N):
        for k in keys[it % len(keys):] + keys[:it % len(keys)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            cands[k]()
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            dev[k].append(e0.elapsed_time(e1) * 1e-3)
            host[k].append(t1 - t0)
    return dev, host


@torch.no_grad()
def main():
    L = _cabi.lib()
    lines = []
    g = torch.Generator().manual_seed(0)
    for case, E, R, C in CASES:
        for tname, t in TYPES:
            bs, ts = ops.block_geometry(t)
            src = torch.randint(0, 256, (E * R * (C // bs) * ts,), dtype=torch.uint8, generator=g).cuda()
            dst = torch.empty(E, R, C, dtype=torch.bfloat16, device="cuda")
            ref = torch.empty(E, R, C, dtype=torch.bfloat16, device="cuda")
            per = [(src.view(E, -1)[e], ref[e], t, None) for e in range(E)]
            ops.level_switch(per)
            ops.level_switch_experts([(src, dst, t)])
            same = bool(torch.equal(dst.view(torch.int16), ref.view(torch.int16)))
            del ref
            per = [(src.view(E, -1)[e], dst[e], t, None) for e in range(E)]
            stream = torch.cuda.current_stream().cuda_stream
            one = (_cabi.SwitchExpertsJob * 1)(_cabi.SwitchExpertsJob(src.data_ptr(), dst.data_ptr(), E, R, C, R * C, t, _cabi.BF16))
            many = (_cabi.SwitchJob * E)(*[_cabi.SwitchJob(s.data_ptr(), d.data_ptr(), None, R, C, t, _cabi.BF16) for s, d, _, _ in per])

            def lib_stacked():
                assert L.gq_level_switch_experts(one, 1, stream) == 0

            def lib_per_expert():
                assert L.gq_level_switch(many, E, stream) == 0

            dev, host = measure({"stacked": lib_stacked, "per_expert": lib_per_expert})
            _, opsh = measure({"stacked": lambda: ops.level_switch_experts([(src, dst, t)]), "per_expert": lambda: ops.level_switch(per)})
            byts = src.numel() + dst.numel() * 2
            rec = {"what": "switch", "case": case, "E": E, "R": R, "C": C, "type": tname, "out": "bf16", "bit_identical": same,
                   "launches": {"stacked": 1, "per_expert": -(-E // _cabi.SWITCH_MAX_JOBS)}}
            for k in ("stacked", "per_expert"):
                rec[k] = {"device": stats(dev[k]), "host": stats(host[k]), "ops": stats(opsh[k]),
                          "GBps": round(byts / statistics.median(dev[k]) / 1e9, 1)}
            rec["stacked_over_per_expert"] = {w: round(rec["stacked"][w]["us"] / rec["per_expert"][w]["us"], 3)
                                              for w in ("device", "host", "ops")}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del src, dst, per, one, many
            torch.cuda.empty_cache()
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
