"""Round 5 GPU tests (VERDICT r04 "next round" items)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------- item 1: bench.py starts its own ranks
@pytest.mark.parametrize("n", [2, 8])
def test_bench_launches_its_own_ranks(n):
    """exactly the driver's command form -- `python3 bench.py --gpus N ...`, no torchrun in front -- must
    run N ranks (reference: run_quant.sh:15 starts them, quant.py:149-155 joins them).  On a box with fewer than N GPUs the
    ranks share the GPU over gloo (asked for explicitly); with N GPUs the same command without --backend runs RCCL."""
    backend = [] if torch.cuda.device_count() >= n else ["--backend", "gloo"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), *backend, "--steps", "1", "--warmup", "1",
           "--workload", "tinyllama-block-q4k", "--full"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1800, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2  # rank 0 only: the full dict, then the compact headline
    full, compact = lines
    for l in lines:
        assert l["n_gpus"] == n and l["ranks_seen"] == n and l["value"] > 0
    assert len(p.stdout.splitlines()[-1]) <= 2048 and p.stdout.splitlines()[-1].startswith("{")
    assert full["collectives_per_step"]["all_gather"] == 1 and full["allreduce_probe"]["ms"] > 0
    assert compact["roofline"]["frac"] > 0 and compact["cpu_baseline"] is None  # the host-core baseline is an N = 1 leg
    assert full["config"]["calib_seqs_per_rank"] == 32 // n
    # nothing on rank 0 may enter a collective the other ranks do not (it would hang under RCCL): the single-GPU side legs are off
    assert all(full[k] is None for k in ("trailing_update", "encoders", "column_loop", "tolerance_parity", "fast_obq"))
    assert "Connection closed" not in json.dumps(full)


def test_bench_refuses_more_ranks_than_gpus_without_gloo():
    """`--gpus N` on a box with fewer GPUs and no explicit gloo: refuse (non-zero exit, nothing measured) instead of
    printing an n_gpus = 1 line."""
    n = torch.cuda.device_count() + 1
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode != 0 and "RCCL needs one GPU per rank" in p.stderr and "{" not in p.stdout


def test_bench_rank_mismatch_is_fatal():
    """A launcher that started ONE rank for `--gpus 2` must not produce a line."""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--workload", "tinyllama-block-q4k"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode != 0 and "rank(s) answered" in p.stderr and "{" not in p.stdout


# ----------------------------------------------------------------- item 2: the row split is exact
def test_row_split_slice_without_a_valid_group_falls_back_to_the_whole_matrix():
    """VERDICT r04 next #2 on the HIP library: 4 gloo ranks share the GPU; a Linear split 128 rows per rank whose second
    slice is ~2e-8 (no group of it is ever `valid`, quant_utils.py:250-252).  gq_gptq_quantize_slice reports the panel-wide
    re-search of that slice, the count rides in the block's ONE all-gather, every rank quantizes the whole matrix: the
    bytes of owner mode (GQ_ROW_SPLIT=0), which are the oracle's bytes for (W, U).  Ordinary weights: nothing redone."""
    import torch.multiprocessing as mp
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_host_logic_cpu as hl
    world = 4
    mgr = mp.Manager()
    got = {}
    for k, (mode, tiny) in enumerate((("0", True), ("all", True), ("all", False), ("0", False))):
        ret = mgr.dict()
        mp.spawn(hl._worker_rowsplit_corner, args=(world, 36000 + 13 * k + os.getpid() % 2000, ret, mode, tiny, True, "cuda:0"),
                 nprocs=world, join=True)
        got[(mode, tiny)] = [ret[r] for r in range(world)]
    for tiny in (True, False):
        ref = got[("0", tiny)][0][0]
        for r in range(world):
            for mode in ("0", "all"):
                assert all(torch.equal(a, b) for a, b in zip(ref, got[(mode, tiny)][r][0])), f"rank {r} mode {mode} tiny {tiny}"
    for r in range(world):
        assert got[("all", True)][r][1] == 1 and got[("all", False)][r][1] == 0
        coll = got[("all", True)][r][2]
        assert (coll["all_gather"], coll["broadcast"], coll.get("small_all_reduce", 0)) == (1, 0, 0), coll


def test_slice_entry_counts_panel_researches_like_the_oracle():
    """gq_gptq_quantize_slice against the oracle's instrumented make_k_quants on the same (W, U): same ints, same count of
    skipped-iterations-with-a-taker -- zero on weight-like rows, positive on a slice of ~1e-8 rows."""
    from gptq_gguf_toolkit_amd import ops
    from oracle import oracle as O
    torch.manual_seed(3)
    R, C = 128, 512
    Z = torch.randn(C, 2 * C).double()
    U = torch.linalg.cholesky(torch.linalg.inv(Z @ Z.T / C + torch.eye(C).double()), upper=True).float().cuda().contiguous()
    for scale, want_positive in ((0.02, False), (2e-8, True)):
        W = (torch.randn(R, C) * scale).cuda()
        n = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        Wg = W.clone()
        q, d, s, dmin, m = ops.gptq_quantize(Wg, U, 12, 128, panel_researches=n)
        O.panel_researches(reset=True)
        _, oq, od, os_, odm, om = O.gptq_step(W.cpu().numpy(), U.cpu().numpy(), 12, block_size=128)
        cnt = O.panel_researches(reset=True)
        assert int(n.item()) == cnt and (cnt > 0) == want_positive, (int(n.item()), cnt)
        assert (q.cpu().numpy() == oq).all() and (s.cpu().numpy() == os_).all() and (m.cpu().numpy() == om).all()


# ----------------------------------------------------------------- RCCL API surface (what one GPU can show)
_RCCL_ONE = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, {root!r})
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT={port!r}, RANK="0", WORLD_SIZE="1")
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", device_id=dev)            # bench.py / quant.py: exactly this call
from gptq_gguf_toolkit_amd import dist_utils
assert dist.get_backend() == "nccl"
C = 1024
H = torch.randn(C, C, device=dev); H = H + H.T
ref = H.clone()
# the calls the N > 1 path issues, forced past the world-size-1 shortcuts: payload dtypes, ops and tensor forms RCCL must take
from gptq_gguf_toolkit_amd import ops
p = ops.h_pack_upper(H)
dist.all_reduce(p, op=dist.ReduceOp.AVG)                   # gptq.py:131-132
dist.reduce(p, dst=0, op=dist.ReduceOp.AVG)                # reduce to owner
dist.reduce(p, dst=0, op=dist.ReduceOp.SUM)
ops.h_unpack_upper(p, H)
assert torch.equal(H, ref)
cnt = torch.zeros(1, dtype=torch.float64, device=dev); dist.all_reduce(cnt, op=dist.ReduceOp.SUM)      # MoE sample counts
n32 = torch.zeros(1, dtype=torch.int32, device=dev); dist.all_reduce(n32, op=dist.ReduceOp.SUM)        # row-split re-search counts
buf = (torch.arange(4096, device=dev) % 251).to(torch.uint8)
out = dist_utils.all_gather_bytes(buf, 4096)               # ONE all-gather per block: uint8 all_gather_into_tensor
assert out.shape == (1, 4096) and torch.equal(out[0], buf)
lo = torch.ones(1, device=dev, dtype=torch.float64); dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(lo, op=dist.ReduceOp.MAX)
box = ["x"]; dist.broadcast_object_list(box, src=0)        # bench.py whole-model leg: the save directory
dist.barrier(); torch.cuda.synchronize()
dist.destroy_process_group()
print("RCCL-ONE-OK")
"""


def test_rccl_collectives_the_path_issues_are_accepted_on_one_rank():
    """N > 1 over RCCL has never been observed (one GPU per box).  What one GPU can show: every collective CALL the N > 1 path
    issues -- backend init with device_id, all_reduce / reduce with AVG on the packed fp32 Hessian tiles, fp64 and int32 SUM,
    uint8 all_gather_into_tensor, MIN / MAX, broadcast_object_list, barrier -- is accepted by RCCL with these dtypes and ops
    (a one-rank communicator), so that the first multi-GPU lease cannot die on an unsupported call."""
    code = _RCCL_ONE.format(root=ROOT, port=str(38000 + os.getpid() % 2000))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = env.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "RCCL-ONE-OK" in p.stdout, p.stderr[-3000:]
