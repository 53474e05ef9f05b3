"""One whole expert FFN of a packed MoE layer's decode step on int8 activations (K38) beside the 16-bit decode path and
transformers' loop, and the kernel's two A/Bs: one JSON line per point.
  q8   PackedExperts.forward with decode_act = "q8"   -- K38: three gq_gemv_packed_experts_a8 launches, SwiGLU in the third's prologue
  fp   the same module with decode_act = "fp"         -- K24: three gq_gemv_packed_experts launches and gq_fwd_silu_mul
  hf   transformers' MixtralExperts.forward           -- on the decoded bf16 weights, host synchronisations included (Q4_K, Q6_K)
at Mixtral-8x7B's shapes (E = 8, K = 2, H = 4096, I = 14336, bf16): Q4_K and Q6_K at T in {1, 2, 4}, the other four types at
T = 1.  `kernel` lines time ONE launch (gate: [14336, 4096], pairs_per_row = K; down: [4096, 14336], pairs_per_row = 1 with
x_up) and give the algorithmic GB/s of the hit experts' bytes; with --variant NAME=LIB (repeatable) the same launch is timed
through other builds of the library in the same process, alternating with the shipped one -- the A/Bs of DESIGN K38:
    make -C gptq-gguf-toolkit_amd/csrc CXXFLAGS='<the Makefile's> -DGQ_GEMV_EXPERTS_A8_GRID_X_CAP=64'   (and 256)
    make -C gptq-gguf-toolkit_amd/csrc CXXFLAGS='<the Makefile's> -DGQ_GEMV_EXPERTS_A8_IDLE_COLUMNS'
each copied aside as NAME.so.  Method, `measure`, `hf_experts` and the cold-weight rotation are profiles/moe_gemv_rate.py's (one
process, HIP events around M back-to-back calls behind a blocker, candidates alternating, median of N with min-max).
usage: python profiles/moe_gemv_a8_rate.py [N=15] [--out FILE] [--variant NAME=LIB ...]   (GPU box; needs only the built tree)."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
argv = sys.argv[1:]
OUT = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(HERE, "moe_gemv_a8_rate.txt")
VARIANTS = dict(argv[i + 1].split("=", 1) for i, a in enumerate(argv) if a == "--variant")
import moe_gemv_rate as base  # noqa: E402
import torch  # noqa: E402
from gptq_gguf_toolkit_amd import _cabi, ops  # noqa: E402
from gptq_gguf_toolkit_amd.ops import _DT, _ptr, _stream  # noqa: E402
from gptq_gguf_toolkit_amd.packed_experts import ROLES, PackedExperts  # noqa: E402

base.N = int(argv[0]) if argv and argv[0].isdecimal() else 15
NAMES = {12: "Q4_K", 14: "Q6_K", 10: "Q2_K", 11: "Q3_K", 13: "Q5_K", 8: "Q8_0"}
FULL = (12, 14)  # every T and the hf column; they come first
E, K, H, I, COPIES, DT = base.E, base.K, base.H, base.I, base.COPIES, base.DT


def bind(path):
    L = ctypes.CDLL(path)
    L.gq_gemv_packed_experts_a8.argtypes = _cabi.lib().gq_gemv_packed_experts_a8.argtypes
    return L


def launch(L, t, blocks, R, x, up, pairs, ppr, y):
    rc = L.gq_gemv_packed_experts_a8(t, _ptr(blocks), E, R, x.shape[1], _ptr(x), _ptr(up), x.shape[0], _ptr(pairs), pairs.numel(),
                                     ppr, _DT[x.dtype], _ptr(y), _stream(x))
    assert rc == 0, rc


@torch.no_grad()
def main():
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        with open(OUT, "w") as f:  # (after every line: a run that is cut short keeps what it measured)
            f.write("\n".join(lines) + "\n")

    libs = dict({"shipped": _cabi.lib()}, **{k: bind(v) for k, v in VARIANTS.items()})
    g = torch.Generator(device="cuda").manual_seed(0)
    big = torch.randn(16384, 8192, device="cuda", generator=g).to(DT)
    blocker = lambda: torch.mm(big, big[:8192])  # noqa: E731
    hf, hf_loop = base.hf_experts()
    for t in NAMES:
        layers, dense = [], []
        for c in range(COPIES):
            mod = PackedExperts(E, H, I, DT)
            for role in ROLES:
                R, C = mod.role_shape(role)
                W = torch.randn(E * R, C, device="cuda", generator=g) * 0.02
                mod.set_level(role, (ops.quantize_q8_0(W) if t == 8 else ops.pack(t, *ops.rtn_quantize(W, t))).view(-1), t)
                del W
            layers.append(mod)
            if t in FULL:
                dense.append((mod.dense_gate_up(), mod.dense_weight("down")))
        role_bytes = {r: layers[0].levels[r][0].numel() // E for r in ROLES}
        for T in ((1, 2, 4) if t in FULL else (1,)):
            x = torch.randn(T, H, device="cuda", generator=g).to(DT)
            w, idx = torch.topk(torch.rand(T, E, device="cuda", generator=g), K, -1)  # uniformly random distinct experts
            w = w / w.sum(-1, keepdim=True)
            hit = int(idx.unique().numel())

            def run(i, act):
                mod = layers[i % COPIES]
                mod.decode_act = act
                return mod(x, idx, w)

            def hf_call(i):
                hf.gate_up_proj, hf.down_proj = dense[i % COPIES]
                return hf_loop(hf, x, idx, w)

            layers[0].decode_act = "q8"
            assert layers[0].takes_q8_decode_path(T, K)
            cands = {"q8": lambda i: run(i, "q8"), "fp": lambda i: run(i, "fp")}
            if t in FULL:
                cands["hf"] = hf_call
            diff = float((run(0, "q8").float() - run(0, "fp").float()).abs().max() / run(0, "fp").float().abs().max())
            m = base.measure(cands, blocker)
            nbytes = hit * sum(role_bytes.values())
            row = {"ffn": NAMES[t], "E": E, "K": K, "H": H, "I": I, "T": T, "dtype": "bf16", "experts_hit": hit,
                   "hit_MB": round(nbytes / 1e6, 1), "calls": base.N * base.M, "copies": COPIES,
                   **{k: base.us(v) for k, v in m.items()}, "q8_GBs": round(nbytes / m["q8"][0] / 1e9),
                   "q8_over_fp": round(m["q8"][0] / m["fp"][0], 3), "diff": round(diff, 5)}
            if "hf" in m:
                row["q8_over_hf"] = round(m["q8"][0] / m["hf"][0], 3)
            emit(row)

            # ---- one launch alone, through every build of the library
            pairs = idx.reshape(-1).to(torch.int32)
            gate = ops.gemv_packed_experts_q8(t, layers[0].levels["gate"][0], E, I, x, pairs, K)
            up = ops.gemv_packed_experts_q8(t, layers[0].levels["up"][0], E, I, x, pairs, K)
            for role, R, inp, xup, ppr in (("gate", I, x, None, K), ("down", H, gate, up, 1)):
                y = torch.empty(T * K, R, dtype=DT, device="cuda")
                m = base.measure({k: (lambda i, L=L: launch(L, t, layers[i % COPIES].levels[role][0], R, inp, xup, pairs, ppr, y))
                                  for k, L in libs.items()}, blocker)
                emit({"kernel": NAMES[t], "role": role, "R": R, "C": inp.shape[1], "T": T, "experts_hit": hit,
                      **{k: dict(base.us(v), GBs=round(hit * role_bytes[role] / v[0] / 1e9)) for k, v in m.items()}})
        hf.gate_up_proj = hf.down_proj = None
        del layers, dense
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
