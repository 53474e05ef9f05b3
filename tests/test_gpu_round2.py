"""-m gpu, round 2: the parity holes VERDICT r01 listed.
  * G1 (edge rows: constants, zeros, denormals, the D <= eps region) and G3 (.5 ties, the eps clamp) THROUGH the
    HIP kernels, bit for bit against the reference's outputs;
  * full BASELINE shapes through gq_gptq_quantize against oracle row slices given the same U: config 2
    (gate/up 14336x4096, down 4096x14336), TinyLlama (C = 2048 / 5632) and Llama-3-70B (C = 8192, R = 28672);
  * tolerance-class stages with their measured rates: GPU H -> U -> ints vs the fp64 chain, and the split-bf16
    Cholesky's accuracy at C = 14336 as an assertion;
  * the block scheduler of the package (the schedule bench.py measures) against per-handle quantize();
  * two ranks: bench.py --gpus 2 with GQ_BENCH_VERIFY=1 (nccl when the box has 2 GPUs, else gloo ranks sharing
    the GPU) and the reference's own 2-rank run (G13).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, triu_unpack

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TYPES = {"Q2_K": 10, "Q3_K": 11, "Q4_K": 12, "Q5_K": 13, "Q6_K": 14}
GROUP = {"Q2_K": 16, "Q3_K": 16, "Q4_K": 32, "Q5_K": 32, "Q6_K": 16}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from gptq_gguf_toolkit_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u16(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def npy(t):
    return t.cpu().numpy()


def f16t(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.float16).cuda()


def bits_eq(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


# ----------------------------------------------------------------- G1 through gq_group_search
@pytest.mark.parametrize("wide", ["0", "1", "2"])
@pytest.mark.parametrize("name", list(TYPES))
def test_g1_group_search_golden(ops, name, wide):
    """make_k_quants / make_quants (quant_utils.py:147-274) on the reference's G1 groups -- incl. the all-equal,
    all-zero, denormal, one-outlier and 1e-7 (D <= eps) rows -- fed as [rows, 256] panels to every mapping of the
    HIP search kernel: group scales and zeros bit-identical to the reference's (incl. -0.0)."""
    g = load_golden("g1_make_quants")
    x = g[f"{name}_x"]
    G = GROUP[name]
    panels = dev(x.reshape(-1, 256))
    _opt = ops.options(ss_wide=int(wide)).__enter__()  # the kernel mapping under test
    try:
        gs, gz, *_ = ops.group_search(panels, TYPES[name])
    finally:
        _opt.__exit__()
    assert bits_eq(npy(gs).ravel(), g[f"{name}_ieee_scale"]), "group scales differ from the reference"
    assert bits_eq(npy(gz).ravel(), g[f"{name}_ieee_zero"]), "group zeros differ from the reference"


def test_g1_search_params_on_gpu(ops):
    g = load_golden("g1_make_quants")
    x = dev(g["Q4_K_alt_x"].reshape(-1, 256))
    gs, gz, *_ = ops.group_search(x, 12, rmin=-0.5, rdelta=0.05, nstep=10)
    assert bits_eq(npy(gs).ravel(), g["Q4_K_alt_scale"]) and bits_eq(npy(gz).ravel(), g["Q4_K_alt_zero"])
    gs, gz, *_ = ops.group_search(x, 12, nstep=0)
    assert bits_eq(npy(gs).ravel(), g["Q4_K_nstep0_scale"]) and bits_eq(npy(gz).ravel(), g["Q4_K_nstep0_zero"])


# ----------------------------------------------------------------- G3 through the column-loop / dequantize kernels
@pytest.mark.parametrize("name", list(TYPES))
def test_g3_elementwise_on_gpu(ops, name):
    """quantize / dequantize (quant_utils.py:34-46) incl. exact .5 ties and the d*s = 0 eps clamp.  Row i of a
    [4096, 256] matrix carries G3's (x_i, d_i, s_i, dmin_i, m_i) in column 0 with U = I, so the column-loop kernel
    (static scales given: the act_order entry with the identity permutation) computes exactly quantize(x_i) and
    leaves dequantize(q_i) in W; gq_dequantize is checked on the same tuples.  Q3_K has no static-scale entry
    (gptq.py:204-206): its quantize arithmetic is the shared device function, its dequantize is checked."""
    g = load_golden("g3_elementwise")
    t, G = TYPES[name], GROUP[name]
    x, d, dmin, s, m, qref, wref = (g[f"{name}_{k}"] for k in ("x", "d", "dmin", "s", "m", "q", "w"))
    n = x.shape[0]
    sdt = s.dtype
    S = np.ones((n, 256 // G), sdt)
    M = np.zeros((n, 256 // G), sdt)
    S[:, 0], M[:, 0] = s, m
    dd, dm = f16t(d.reshape(n, 1)), f16t(dmin.reshape(n, 1))
    Sd, Md = dev(S), dev(M)
    if name != "Q3_K":
        W = torch.zeros(n, 256, device="cuda")
        W[:, 0] = dev(x)
        U = torch.eye(256, device="cuda")
        perm = torch.arange(256, device="cuda", dtype=torch.int32)
        q = ops.gptq_quantize_perm(W, U, t, perm, dd, Sd, dm, Md, block_size=128)
        assert np.array_equal(npy(q)[:, 0].astype(np.float32), qref), \
            f"{(npy(q)[:, 0].astype(np.float32) != qref).mean():.4%} of G3's quantize() results differ"
        assert bits_eq(npy(W)[:, 0], wref), "W[:, 0] after the column loop != dequantize(quantize(x))"
    # a11 (quant_utils.py:277-310) starts from the STORED ints: the float -0.0 that round() gives for tiny negative
    # inputs is 0 there, so dequantize(ints) == G3's w everywhere except the sign of those zeros
    Q = torch.zeros(n, 256, device="cuda", dtype=torch.int8 if sdt == np.int8 else torch.uint8)
    Q[:, 0] = dev(qref.astype(np.int8 if sdt == np.int8 else np.uint8))
    got = npy(ops.dequantize(t, Q, dd, Sd, dm, Md))[:, 0]
    qi = qref.astype(np.int8 if sdt == np.int8 else np.uint8).astype(np.float32)
    want = (d.view(np.float16).astype(np.float32) * s.astype(np.float32)) * qi \
        - dmin.view(np.float16).astype(np.float32) * m.astype(np.float32)
    assert np.array_equal(want, wref) and np.array_equal(np.signbit(want) != np.signbit(wref), (qref == 0) & np.signbit(qref) & (wref == 0))
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (f"gq_dequantize differs from the reference's dequantize() at {bad.size} of {n}: "
                           + "; ".join(f"i={i} got={got[i]!r} want={want[i]!r} q={qref[i]} d={d[i]} s={s[i]} "
                                       f"dmin={dmin[i]} m={m[i]}" for i in bad[:6]))


# ----------------------------------------------------------------- full BASELINE shapes vs oracle row slices
def _hessian(ops, C, T, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sig = torch.exp(torch.randn(C, device="cuda", generator=g) * 0.5)
    sig[torch.randperm(C, device="cuda", generator=g)[:max(1, C // 1000)]] *= 20.0  # outlier channels
    H = torch.zeros(C, C, device="cuda")
    done = 0
    while done < T:
        b = min(8192, T - done)
        X = (torch.randn(b, C, device="cuda", generator=g) * sig).half()
        ops.h_accumulate(H, X, done / (done + b), 2.0 / (done + b))
        done += b
    return H


@pytest.mark.parametrize("tag,R,C,name,rows", [
    ("llama3-8b gate/up", 14336, 4096, "Q4_K", (9001, 9033)),
    ("llama3-8b down", 4096, 14336, "Q4_K", (2050, 2066)),
    ("tinyllama down", 2048, 5632, "Q4_K", (1000, 1032)),     # 5.5 look-ahead super-blocks
    ("tinyllama gate/up", 5632, 2048, "Q4_K", (5600, 5632)),  # last rows of a 64-row workgroup tail
    ("llama3-70b q/o", 8192, 8192, "Q4_K", (4097, 4113)),
    ("llama3-70b gate/up", 28672, 8192, "Q4_K", (28650, 28672)),
    ("mixtral w2 Q3_K", 4096, 14336, "Q3_K", (77, 93)),
])
def test_full_shape_column_loop_vs_oracle_rows(ops, oracle, tag, R, C, name, rows):
    """The whole gq_gptq_quantize (lazy scale search at every 256-column boundary, column-loop kernel, near and
    chained far trailing updates) at the FULL shape; rows are independent given U, so a row slice through the
    oracle with the same (W, U) must agree bit for bit in ints, scales and final weights."""
    t = TYPES[name]
    H = _hessian(ops, C, min(2 * C, 16384), seed=R + C)
    g = torch.Generator(device="cuda").manual_seed(R * 7 + C)
    W0 = (torch.randn(R, C, device="cuda", generator=g) * 0.02).half().float()
    Wp = W0.clone()
    U, flag = ops.h_prepare(H, Wp, 0.01)
    assert int(flag.item()) == 0
    del H
    W = Wp.clone()
    q, d, s, dmin, m = ops.gptq_quantize(W, U, t, block_size=128)
    r = slice(*rows)
    Wd, oq, od, os_, odm, om = oracle.gptq_step(npy(Wp[r]), npy(U), t, block_size=128)
    assert np.array_equal(npy(q[r]), oq), f"{tag}: {(npy(q[r]) != oq).mean():.4%} ints differ"
    assert np.array_equal(u16(d[r]), od) and np.array_equal(u16(dmin[r]), odm)
    assert np.array_equal(npy(s[r]), os_) and np.array_equal(npy(m[r]), om)
    assert np.array_equal(npy(W[r]), Wd)
    assert torch.equal(W, ops.dequantize(t, q, d, s, dmin, m))  # gptq.py:266 on every row


# ----------------------------------------------------------------- tolerance-class stages, measured
def test_end_to_end_rates_vs_fp64_chain(ops, oracle):
    """K1 (MFMA SYRK) and K3 (split-bf16 / fp32 Cholesky chain) are tolerance-class.  Their end-to-end effect at
    4096 x 4096 Q4_K: the GPU's H -> U -> ints against fp64 H -> fp64 LAPACK chain -> oracle column loop on the
    same inputs.  Asserted: measured rates + margin; printed for the record."""
    C = R = 4096
    T = 16384
    g = torch.Generator(device="cuda").manual_seed(21)
    sig = torch.exp(torch.randn(C, device="cuda", generator=g) * 0.5)
    sig[torch.randperm(C, device="cuda", generator=g)[:4]] *= 20.0
    X = (torch.randn(T, C, device="cuda", generator=g) * sig).half()
    W0 = (torch.randn(R, C, device="cuda", generator=g) * 0.02).half().float()
    H = torch.zeros(C, C, device="cuda")
    ops.h_accumulate(H, X, 0.0, 2.0 / 8)
    Wg = W0.clone()
    U, flag = ops.h_prepare(H.clone(), Wg, 0.01)
    assert int(flag.item()) == 0
    q, d, s, dmin, m = ops.gptq_quantize(Wg, U, 12, 128)
    H64 = (2.0 / 8) * (X.double().T @ X.double())  # fp64 reference of the Hessian (torch, on the GPU)
    h_err = float((H.double() - H64).abs().max() / H64.abs().max())
    Hd = H64.clone()  # gptq.py:304-324 in fp64 (no dead channel / zero column in this input)
    Hd.diagonal().add_(0.01 * Hd.diagonal().mean())
    Uo = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(Hd)), upper=True).cpu().numpy()
    Wo = npy(W0)
    u_err = float(np.abs(npy(U).astype(np.float64) - Uo).max() / np.abs(Uo).max())
    rows = slice(0, 1024)  # the oracle walks 1024 of the 4096 independent rows
    U32 = Uo.astype(np.float32)
    Wd, oq, od, os_, odm, om = oracle.gptq_step(Wo[rows], U32, 12, block_size=128)

    def rates(q_, d_, s_, dmin_, m_):
        sc_ = np.concatenate([(d_ != od).ravel(), (s_ != os_).ravel(), (dmin_ != odm).ravel(), (m_ != om).ravel()])
        return float((q_ != oq).mean()), float(sc_.mean())

    ints, sc = rates(npy(q[rows]), u16(d[rows]), npy(s[rows]), u16(dmin[rows]), npy(m[rows]))
    dw = float(np.abs(npy(Wg[rows]) - Wd).max())
    # the noise floor of the comparison: the same oracle with U perturbed by 1e-7 relative (below one fp32
    # rounding).  The column loop's error feedback amplifies any last-bit difference over 4096 dependent steps.
    rng = np.random.default_rng(0)
    Un = (Uo * (1.0 + 1e-7 * rng.standard_normal(Uo.shape))).astype(np.float32)
    _, nq, nd, ns, ndm, nm = oracle.gptq_step(Wo[rows], Un, 12, block_size=128)
    f_ints, f_sc = rates(nq, nd, ns, ndm, nm)
    print(f"\n[tolerance] 4096x4096 Q4_K vs fp64 chain: H rel err {h_err:.2e}, U rel err {u_err:.2e}, "
          f"ints differ {ints:.4%} (1e-7-noise floor {f_ints:.4%}), scale bytes differ {sc:.4%} (floor {f_sc:.4%}), "
          f"max |dW| {dw:.3e}")
    # r03: tightened -- a 2x loss of Cholesky accuracy now fails both lines.  Measured on the r03
    # build: U 2.5e-7 (r02: 3.4e-7), ints 1.60 x floor, scale bytes 1.55 x floor.
    assert h_err < 5e-7 and u_err < 6e-7
    assert ints < 1.7 * f_ints and sc < 1.7 * f_sc, (ints, f_ints, sc, f_sc)
    assert dw < 0.05


def test_cholesky_chain_accuracy_full_size(ops):
    """gq_h_prepare at C = 14336 (image GEMMs at the three top levels, fp32 below) against torch's fp64 chain on the GPU:
    max |U - U64| / max |U64| as an assertion (r01: a probe, 2.8e-7 on an outlier-channel Hessian)."""
    C = 14336
    H = _hessian(ops, C, 2 * C, seed=5)
    W = torch.randn(64, C, device="cuda")
    Hd = H.clone()
    U, flag = ops.h_prepare(Hd, W, 0.01)  # Hd now holds the damped matrix
    assert int(flag.item()) == 0
    U64 = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(Hd.double())), upper=True)
    err = float((U.double() - U64).abs().max() / U64.abs().max())
    print(f"\n[tolerance] h_prepare(14336): max|U-U64|/max|U64| = {err:.2e}")
    assert err < 1e-6, err  # r03: 3.2e-7 with the row-scaled fp16 image GEMMs on the equilibrated matrix (r02: 1.1e-6)


# ----------------------------------------------------------------- the package's block scheduler
def _toy_block(seed=0, dims=((512, 512, "a"), (256, 512, "a"), (256, 512, "a"), (512, 512, "o"), (1024, 512, "m"),
                             (1024, 512, "m"), (512, 1024, "d")), L=96, n_samples=6):
    names = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]
    g = torch.Generator(device="cuda").manual_seed(seed)
    layers, inputs = {}, {}
    for n, (R, C, grp) in zip(names, dims):
        lin = torch.nn.Linear(C, R, bias=False, device="cuda", dtype=torch.float16)
        lin.weight.data = (torch.randn(R, C, device="cuda", generator=g) * 0.02).half()
        layers[n] = lin
        if grp not in inputs:
            sig = torch.exp(torch.randn(C, device="cuda", generator=g) * 0.5)
            inputs[grp] = [(torch.randn(1, L, C, device="cuda", generator=g) * sig).half() for _ in range(n_samples)]
    return layers, {n: inputs[grp] for n, (_, _, grp) in zip(names, dims)}


def test_block_schedule_equals_per_handle_quantize(ops):
    """BlockSchedule (grouped SYRK flushes, shared Hessians, one chain per input on its own HIP stream, speculative
    reuse of the leader's U) must give exactly what the reference's loop gives -- one handle after the other,
    each with its own update() calls and quantize() (quantizer.py:248-265)."""
    from gptq_gguf_toolkit_amd.block_schedule import BlockSchedule
    from gptq_gguf_toolkit_amd.gptq import GPTQ
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    qt = {"q_proj": T.Q3_K, "k_proj": T.Q2_K, "v_proj": T.Q4_K, "o_proj": T.Q5_K, "gate_proj": T.Q6_K,
          "up_proj": T.Q4_K, "down_proj": T.Q3_K}
    layers, xs = _toy_block()
    W0 = {n: l.weight.data.clone() for n, l in layers.items()}
    sched = BlockSchedule(layers, lambda l, n: GPTQ(l, rel_damp=0.01, block_size=128))
    for h in sched.handles.values():
        h.flush_tokens = 192  # several grouped flushes over the 6 x 96 tokens
    for i in range(6):
        for n in layers:
            sched.feed(n, xs[n][i])
        sched.sample_done()
    out = sched.quantize(qt, writeback=True)
    torch.cuda.synchronize()
    assert sched.stats["reused_U"] == 3 and sched.stats["refactorised"] == 0 and sched.stats["syrk_launches"] >= 3
    for n, l in layers.items():
        ref_layer = torch.nn.Linear(l.in_features, l.out_features, bias=False, device="cuda", dtype=torch.float16)
        ref_layer.weight.data = W0[n].clone()
        h = GPTQ(ref_layer, rel_damp=0.01, block_size=128)
        h.flush_tokens = 192  # the same fold cadence: H is a sum in launch order
        for i in range(6):
            h.update(xs[n][i])
        ref = h.quantize(qt[n])
        for a, b in zip(out[n], ref):
            assert torch.equal(a, b), f"{n}: scheduler result differs from the per-handle path"
        from gptq_gguf_toolkit_amd.quant_utils import dequantize_linear_weight
        assert torch.equal(l.weight.data, dequantize_linear_weight(qt[n], *ref, out_dtype=torch.float16))


def test_block_schedule_follower_with_own_zero_column(ops):
    """A follower whose weight has an all-zero column its leader's does not: the speculative reuse of the leader's
    U is detected (gq_w_prepare flag) and the follower gets its own factorisation (gptq.py:307-313)."""
    from gptq_gguf_toolkit_amd.block_schedule import BlockSchedule
    from gptq_gguf_toolkit_amd.gptq import GPTQ
    from gptq_gguf_toolkit_amd.quant_utils import GGMLQuantizationType as T
    layers, xs = _toy_block(seed=3)
    layers["k_proj"].weight.data[:, 77] = 0
    W0 = layers["k_proj"].weight.data.clone()
    sched = BlockSchedule(layers, lambda l, n: GPTQ(l, rel_damp=0.01, block_size=128))
    for i in range(6):
        for n in layers:
            sched.feed(n, xs[n][i])
        sched.sample_done()
    out = sched.quantize({n: T.Q4_K for n in layers})
    assert sched.stats["refactorised"] == 1 and sched.stats["reused_U"] == 2
    ref_layer = torch.nn.Linear(512, 256, bias=False, device="cuda", dtype=torch.float16)
    ref_layer.weight.data = W0
    h = GPTQ(ref_layer, rel_damp=0.01, block_size=128)
    for i in range(6):
        h.update(xs["k_proj"][i])
    for a, b in zip(out["k_proj"], h.quantize(T.Q4_K)):
        assert torch.equal(a, b)


def test_handle_reset_allows_reuse(ops):
    """reset() returns the handle to its post-__init__ state: a second round of update + quantize
    gives the result of a fresh handle, and no stale U / reduction flag survives."""
    from gptq_gguf_toolkit_amd.gptq import GPTQ
    torch.manual_seed(1)
    lin = torch.nn.Linear(512, 128, bias=False, device="cuda", dtype=torch.float16)
    xa = (torch.randn(1, 300, 512, device="cuda")).half()
    xb = (torch.randn(1, 70000, 512, device="cuda") * 3).half()  # wider than the first buffer allocation
    h = GPTQ(lin, rel_damp=0.01, block_size=128)
    h.flush_tokens = 256
    h.update(xa)
    r1 = h.quantize(12)
    h.reset()
    assert h.H is None and h._reduced is False and h._U_cache is None and h.num_samples == 0
    h.update(xa[:, :10])
    h.update(xb)  # more tokens than _buf has rows: the buffer is re-allocated after the flush
    r2 = h.quantize(12)
    fresh = GPTQ(lin, rel_damp=0.01, block_size=128)
    fresh.update(xa[:, :10])
    fresh.update(xb)
    r3 = fresh.quantize(12)
    assert all(torch.equal(a, b) for a, b in zip(r2, r3)) and not torch.equal(r1[0], r2[0])


# ----------------------------------------------------------------- two ranks
def _spawn_bench(n, backend, extra=()):
    env = dict(os.environ, GQ_BENCH_VERIFY="1", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr",
           "127.0.0.1", "--master-port", str(23000 + os.getpid() % 4000), os.path.join(ROOT, "bench.py"), "--gpus",
           str(n), "--steps", "1", "--warmup", "1", "--workload", "tinyllama-block-q4k", "--backend", backend,
           "--full", "--no-cpu-baseline", "--no-whole-model", "--no-side-legs", *extra]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    full, compact = lines[-2], lines[-1]  # bench.py: the full dict, then the compact headline LAST
    assert compact["n_gpus"] == full["n_gpus"] == n and compact["value"] == full["value"]
    return full, p.stderr


def test_bench_two_ranks_hold_identical_results():
    """bench.py --gpus 2 through torch.distributed.run: RCCL (`nccl`) when the box has two GPUs, otherwise two gloo
    ranks sharing the one GPU (the same N > 1 code path: calibration shards, all-reduce of the upper Hessian tiles,
    owners, broadcast).  GQ_BENCH_VERIFY=1 makes every rank compare checksums of all results."""
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    line, err = _spawn_bench(2, backend)
    assert "verify: all ranks hold identical results" in err
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["allreduce_probe"]["backend"] == backend
    assert line["value"] > 0 and line["schedule"]["allreduce_bytes"] > 0
    owners = line["config"]["owners"]
    assert set(owners.values()) == {0, 1}, owners  # both ranks own matrices


def test_bench_four_ranks_row_split_and_owners():
    """From 4 ranks up the widest matrix is split by rows (every rank factorises the same reduced H and walks its own
    rows, all-gather of the row slices) and the other six are dealt to owners: bench.py --gpus 4, RCCL when the box
    has four GPUs, else four gloo ranks sharing the one GPU; every rank must hold identical results."""
    backend = "nccl" if torch.cuda.device_count() >= 4 else "gloo"
    line, err = _spawn_bench(4, backend)
    assert "verify: all ranks hold identical results" in err
    assert line["n_gpus"] == 4 and line["ranks_seen"] == 4
    owners = line["config"]["owners"]
    assert owners["down_proj"] == "rows/4" and {v for k, v in owners.items() if k != "down_proj"} == {0, 1, 2, 3}, owners


def _g13_gpu_worker(rank, world, port, ret, backend):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_host_logic_cpu as hl
    torch.cuda.set_device(rank % torch.cuda.device_count())
    hl._worker_g13(rank, world, port, ret, device=f"cuda:{rank % torch.cuda.device_count()}", backend=backend)


def test_two_rank_gpu_run_vs_reference_two_rank_golden():
    """G13 on the GPU: the reference's per-rank Hessians -> the build's all-reduce (RCCL with two GPUs, gloo ranks
    sharing the GPU otherwise) -> HIP prepare + column loop on the owner -> broadcast.  Reduced H bit-identical to
    the reference's all_reduce(AVG); results identical on both ranks; ints vs the reference: a rate (fp32 Cholesky)."""
    import torch.multiprocessing as mp
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_host_logic_cpu as hl
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    ctx = mp.get_context("spawn")
    mgr = ctx.Manager()
    ret = mgr.dict()
    mp.spawn(_g13_gpu_worker, args=(2, 25000 + os.getpid() % 2000, ret, backend), nprocs=2, join=True)
    rates = hl.check_g13(ret)
    print(f"\n[two ranks, {backend}] ints differing from the reference's 2-rank run: {rates}")


# ----------------------------------------------------------------- zero-copy Hessian accumulation
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_h_accumulate_segments_equal_contiguous(ops, dt):
    """gq_h_accumulate_segments (the per-sample activation tensors read where they lie) == the same rows in one
    buffer, bit for bit: two problems in one grid, blocks of 256 and 2048 tokens, long enough for the K-split of
    the last round (T >= 8192), beta != 0."""
    torch.manual_seed(7)
    shapes = [(2048, 6, 2048), (4096, 40, 256)]  # (C, blocks, tokens per block)
    Hs_a, Hs_b, Xc, Xl = [], [], [], []
    for C, nb, L in shapes:
        blocks = [(torch.randn(L, C, device="cuda") * (1 + i % 3)).to(dt) for i in range(nb)]
        pad = torch.empty(7 * 16, device="cuda")  # blocks are separate allocations at unrelated addresses
        Xl.append(blocks)
        Xc.append(torch.cat(blocks))
        H0 = torch.randn(C, C, device="cuda")
        H0 = H0 + H0.T
        Hs_a.append(H0.clone())
        Hs_b.append(H0.clone())
        del pad
    ops.h_accumulate_grouped(Hs_a, Xc, [0.25, 0.5], [0.01, 0.02])
    ops.h_accumulate_grouped(Hs_b, Xl, [0.25, 0.5], [0.01, 0.02])
    for a, b in zip(Hs_a, Hs_b):
        assert torch.equal(a, b)
    # one segmented problem next to one contiguous problem
    Ha, Hb = [torch.zeros(2048, 2048, device="cuda"), torch.zeros(4096, 4096, device="cuda")], \
             [torch.zeros(2048, 2048, device="cuda"), torch.zeros(4096, 4096, device="cuda")]
    ops.h_accumulate_grouped(Ha, [Xc[0], Xc[1]], [0.0, 0.0], [1.0, 1.0])
    ops.h_accumulate_grouped(Hb, [Xl[0], Xc[1]], [0.0, 0.0], [1.0, 1.0])
    assert torch.equal(Ha[0], Hb[0]) and torch.equal(Ha[1], Hb[1])
    from gptq_gguf_toolkit_amd._cabi import GQError
    with pytest.raises(GQError, match="multiple of 128"):
        ops.h_accumulate_grouped([torch.zeros(2048, 2048, device="cuda")],
                                 [[torch.zeros(96, 2048, device="cuda", dtype=dt)] * 4], [0.0], [1.0])


def test_handle_zero_copy_and_staged_paths_agree(ops):
    """GPTQ.update keeps references to [L, C] hook tensors (zero copy) or stages ragged / odd inputs into one buffer
    (gq_h_stage): same H either way; an input modified in place after its hook is reported, not silently used."""
    from gptq_gguf_toolkit_amd.gptq import GPTQ
    torch.manual_seed(2)
    lin = torch.nn.Linear(1024, 64, bias=False, device="cuda", dtype=torch.float16)
    xs = [(torch.randn(1, 256, 1024, device="cuda")).half() for _ in range(5)]
    a = GPTQ(lin)
    b = GPTQ(lin)
    b._zero_copy = False
    for x in xs:
        a.update(x)
        b.update(x)
    assert len(a._segs) == 5 and a._staged == 0 and len(b._segs) == 0 and b._staged == 5 * 256
    a.flush()
    b.flush()
    assert torch.equal(a.H, b.H) and a.num_samples == b.num_samples == 5
    # ragged tail: 3 kept blocks, then a 100-token sample -> everything goes through the staging buffer, in order
    c, d = GPTQ(lin), GPTQ(lin)
    d._zero_copy = False
    tail = torch.randn(1, 100, 1024, device="cuda").half()
    for x in xs[:3] + [tail] + xs[3:]:
        c.update(x)
        d.update(x)
    # (r04: kept by reference, in order, and gathered by ONE launch when the fold is due -- gq_h_stage_many)
    assert not c._segs and len(c._rag) == 6 and c._staged == 0 and c._fill == 5 * 256 + 100 and d._staged == 5 * 256 + 100
    c.flush()
    d.flush()
    assert torch.equal(c.H, d.H)
    e = GPTQ(lin)
    e.update(xs[0])
    xs[0].add_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        e.flush()


# ----------------------------------------------------------------- quant_utils.py:250-252, the panel-wide `continue`
@pytest.mark.parametrize("wide", ["0", "1", "2"])
@pytest.mark.parametrize("name", ["Q2_K", "Q4_K", "Q5_K"])
def test_panel_wide_continue(ops, oracle, name, wide):
    """make_k_quants skips a refinement iteration for EVERY group when no group of the [rows, 256] panel has
    D > 1e-9 in it (r01: a documented deviation of the HIP kernel).  Panels where that happens -- every value ~1e-7,
    or every group constant -- must match the oracle (which takes the `continue`) bit for bit, in all three kernel
    mappings; and the skip must matter: the same tiny rows next to ONE ordinary row give other results."""
    t, G = TYPES[name], GROUP[name]
    rng = np.random.default_rng(TYPES[name])
    rows = 301
    tiny = (rng.standard_normal((rows, 256)) * 2e-8).astype(np.float32)  # D <= 1e-9 in every group, every iteration
    const = np.repeat((rng.standard_normal((rows, 256 // G)) * 0.02).astype(np.float32), G, axis=1)
    const[5] = 0.0
    mixed = tiny.copy()
    mixed[17] = (rng.standard_normal(256) * 0.02).astype(np.float32)
    _opt = ops.options(ss_wide=int(wide)).__enter__()  # the kernel mapping under test
    try:
        outs = {}
        for tag, x in (("tiny", tiny), ("const", const), ("mixed", mixed)):
            gs, gz, d, s, dmin, m = ops.group_search(dev(x), t)
            osc, oze = oracle.make_k_quants(x.reshape(-1, G), oracle.type_info(t)["bits"])
            od, os_, odm, om = oracle.scale_search(x, t)
            assert bits_eq(npy(gs).ravel(), osc) and bits_eq(npy(gz).ravel(), oze), f"{tag}: group scales / zeros"
            assert np.array_equal(u16(d), od) and np.array_equal(npy(s), os_), tag
            assert np.array_equal(u16(dmin), odm) and np.array_equal(npy(m), om), tag
            outs[tag] = npy(gs)
        # scale_search (the entry the column loop uses) on a strided view of a wider matrix
        wide_m = np.zeros((rows, 768), np.float32)
        wide_m[:, 256:512] = tiny
        d, s, dmin, m = ops.scale_search(dev(wide_m)[:, 256:512], t)
        od, os_, odm, om = oracle.scale_search(tiny, t)
        assert np.array_equal(u16(d), od) and np.array_equal(npy(s), os_) and np.array_equal(npy(m), om)
    finally:
        _opt.__exit__()
    keep = np.arange(rows) != 17
    if name != "Q5_K":  # (with 5 bits no candidate of these groups ever wins, skipped or not: oracle, both panels)
        assert not np.array_equal(outs["tiny"][keep], outs["mixed"][keep]), "the panel-wide skip changed nothing"


def test_panel_wide_continue_in_the_column_loop(ops, oracle):
    """gq_gptq_quantize / gq_rtn_quantize on a matrix whose second 256-column stripe is ~1e-7 everywhere."""
    rng = np.random.default_rng(9)
    R, C = 192, 768
    W = (rng.standard_normal((R, C)) * 0.02).astype(np.float32)
    W[:, 256:512] = (rng.standard_normal((R, 256)) * 1e-7).astype(np.float32)
    U = np.triu(rng.standard_normal((C, C)).astype(np.float32) * 0.01, 1) + np.eye(C, dtype=np.float32)
    for t in (12, 10):
        Wg = dev(W)
        q, d, s, dmin, m = ops.gptq_quantize(Wg, dev(U), t, block_size=128)
        Wd, oq, od, os_, odm, om = oracle.gptq_step(W, U, t, block_size=128)
        assert np.array_equal(npy(q), oq) and np.array_equal(u16(d), od) and np.array_equal(npy(s), os_)
        assert np.array_equal(u16(dmin), odm) and np.array_equal(npy(m), om) and np.array_equal(npy(Wg), Wd)
        q, d, s, dmin, m = ops.rtn_quantize(dev(W), t)
        oq, od, os_, odm, om = oracle.rtn_quantize(W, t)
        assert np.array_equal(npy(q), oq) and np.array_equal(u16(d), od) and np.array_equal(npy(s), os_)
        assert np.array_equal(npy(m), om)


@pytest.mark.parametrize("tag,dt", [("f16", torch.float16), ("bf16", torch.bfloat16), ("f32", torch.float32)])
def test_quantizer_get_scale_and_zero_in_the_panel_dtype(ops, tag, dt):
    """quant_utils.Quantizer.get_scale_and_zero (quant_utils.py:90-145) on panels in the model dtype -- what
    Quantizer._quant_non_block_module hands it (quantizer.py:300-310): G9 / G8 hold the reference's outputs."""
    from gptq_gguf_toolkit_amd.quant_utils import GGML_QUANT_SIZES, GGMLQuantizationType, Quantizer
    g = load_golden("g8_g9_rtn_dequant")
    W = dev(g["W" if tag == "f32" else f"W_{tag}"]).to(dt)
    pre = "" if tag == "f32" else f"{tag}_"
    for name in ("Q4_K", "Q6_K", "Q2_K"):
        qt = GGMLQuantizationType[name]
        bits, _, smq, G, SG, sdt, _ = GGML_QUANT_SIZES[qt]
        qz = Quantizer()
        qz.configure(bits, smq, G, sdt, SG)
        for sg in range(W.shape[1] // 256):
            d, s, dmin, m = qz.get_scale_and_zero(W[:, sg * 256:(sg + 1) * 256], qt)
            gps = 256 // G
            assert np.array_equal(u16(d), g[f"{pre}{name}_d"][:, sg]) and np.array_equal(u16(dmin), g[f"{pre}{name}_dmin"][:, sg])
            assert np.array_equal(npy(s), g[f"{pre}{name}_s"][:, sg * gps:(sg + 1) * gps])
            assert np.array_equal(npy(m), g[f"{pre}{name}_m"][:, sg * gps:(sg + 1) * gps])


# ----------------------------------------------------------------- quant_scale = "mse" (quant_utils.py:164-191)
@pytest.mark.parametrize("name", ["Q3_K", "Q6_K"])
def test_mse_quant_scale_golden(ops, oracle, name):
    """make_quants' MSE grid search on the GPU against the reference's outputs (G12: weight-like, mid and the wide panel
    where the branch really differs), every kernel mapping; then the whole column loop and the RTN with quant_scale
    = "mse" on a matrix with large values against the oracle."""
    g = load_golden("g12_mse_scale")
    t = TYPES[name]
    for wide in ("0", "1", "2"):
        _opt = ops.options(ss_wide=int(wide)).__enter__()
        try:
            for tag in ("w", "mid", "wide"):
                for mode in ("absmax", "mse"):
                    d, s, dmin, m = ops.scale_search(dev(g[f"{name}_{tag}_x"]), t, quant_scale=mode)
                    assert np.array_equal(u16(d), g[f"{name}_{tag}_{mode}_d"]), (wide, tag, mode)
                    assert np.array_equal(npy(s), g[f"{name}_{tag}_{mode}_s"]), (wide, tag, mode)
        finally:
            _opt.__exit__()
    rng = np.random.default_rng(t)
    R, C = 96, 512
    W = (rng.standard_normal((R, C)) * 20.0).astype(np.float32)
    U = np.triu(rng.standard_normal((C, C)).astype(np.float32) * 0.01, 1) + np.eye(C, dtype=np.float32)
    try:
        oracle.set_quant_scale("mse")
        Wd, oq, od, os_, odm, om = oracle.gptq_step(W, U, t, block_size=128)
        rq, rd, rs, rdm, rm = oracle.rtn_quantize(W, t)
    finally:
        oracle.set_quant_scale("absmax")
    Wg = dev(W)
    q, d, s, dmin, m = ops.gptq_quantize(Wg, dev(U), t, block_size=128, quant_scale="mse")
    assert np.array_equal(npy(q), oq) and np.array_equal(u16(d), od) and np.array_equal(npy(s), os_) and np.array_equal(npy(Wg), Wd)
    q, d, s, dmin, m = ops.rtn_quantize(dev(W), t, quant_scale="mse")
    assert np.array_equal(npy(q), rq) and np.array_equal(u16(d), rd) and np.array_equal(npy(s), rs)
    qa, da, sa, _, _ = ops.rtn_quantize(dev(W), t)
    assert not np.array_equal(npy(sa), npy(s))  # the mode matters on this matrix


def test_gptq_quantize_random_small_shapes_vs_oracle(ops, oracle):
    """A seeded sweep over ragged row counts (1 .. 257: partial workgroups), widths, block sizes (16 .. C: one segment,
    several segments, the block scratch path), every K-quant type, lazy and static groups and search settings:
    integers, scale ints, fp16 super-scales and the final W against the oracle on the same (W, U), bit for bit."""
    rng = np.random.default_rng(77)
    for case in range(30):
        name = list(TYPES)[case % 5]
        C = int(rng.choice([256, 512, 768, 1280]))
        R = int(rng.choice([1, 5, 63, 64, 65, 129, 257]))
        block = int(rng.choice([16, 32, 64, 128, 256, 384, 0]))
        static = bool(rng.integers(2))
        nstep = int(rng.choice([20, 20, 7, 0]))
        X = rng.standard_normal((2 * C, C)).astype(np.float32) * np.exp(rng.standard_normal(C) * 0.5).astype(np.float32)
        H = dev((2.0 / X.shape[0]) * (X.T @ X))
        W = dev((rng.standard_normal((R, C)) * 0.05).astype(np.float32))
        if case % 4 == 0:
            W[:, int(rng.integers(C))] = 0.0
        U, flag = ops.h_prepare(H, W, 0.01)
        assert int(flag.item()) == 0
        W0, Un = npy(W), npy(U)
        q, d, s, dmin, m = ops.gptq_quantize(W, U, TYPES[name], block, static, nstep=nstep)
        Wd, oq, od, os_, odm, om = oracle.gptq_step(W0, Un, TYPES[name], block_size=block, static_groups=static, nstep=nstep)
        tag = f"case {case}: {name} R={R} C={C} block={block} static={static} nstep={nstep}"
        assert np.array_equal(npy(q), oq), tag
        assert np.array_equal(npy(s), os_) and np.array_equal(npy(m), om), tag
        assert np.array_equal(u16(d), od) and np.array_equal(u16(dmin), odm), tag
        assert bits_eq(npy(W), Wd), tag
