"""GPTQ's column walk on the IQ4_XS / IQ4_NL grid as include/gptq_gguf_iq4_gptq.h states it, restated as loops: over blocks,
over the columns of a block, one operation at a time in np.float32 (the rows are independent and go through numpy together).
The trailing update, a k-ordered fmaf chain, runs through tests/fma_chain.cpp (numpy has no exact fp32 fma).

The scale search of a 256-column group comes in two forms with the same outputs:
  loop_scales  tests/iq4_encode_spec.py's loops (block_scale and the weights / ms / D / l of encode_superblock), element by
               element -- the restatement of the header;
  host_scales  gguf_writer.iq4_scales, the vectorised host form that tests/test_iq4_encode_cpu.py pins to those loops byte for
               byte.  It is what the GPU tests use (the loops take minutes at their shapes); tests/test_iq4_gptq_cpu.py runs
               the walk under both and requires the same outputs.
Nothing here comes from the kernel."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iq4_encode_spec as ES  # noqa: E402

NL, XS = ES.NL, ES.XS
F = np.float32
KVF = np.array(ES.KV, np.float32)
_exe = None


def _fma_exe():
    global _exe
    if _exe is None:
        d = tempfile.mkdtemp(prefix="fma_chain")
        _exe = os.path.join(d, "fma_chain")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall",
                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "fma_chain.cpp"), "-o", _exe])
    return _exe


def trailing_update(W, E, U):
    """W [R, N] - E [R, K] @ U [K, N]: per element a k-ordered fmaf chain from 0, then one subtraction."""
    R, K = E.shape
    N = U.shape[1]
    if N == 0:
        return W
    msg = struct.pack("<3q", R, K, N) + b"".join(np.ascontiguousarray(a, np.float32).tobytes() for a in (E, U, W))
    out = subprocess.run([_fma_exe()], input=msg, stdout=subprocess.PIPE, check=True).stdout
    return np.frombuffer(out, np.float32).reshape(R, N).copy()


def _h2f(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)


def _f2h_bits(v):
    return np.asarray(v, np.float32).astype(np.float16).view(np.uint16)  # round-to-nearest-even


def best(a):
    """best() of gptq_gguf_iq4_encode.h on an fp32 vector: ES.best element by element."""
    return np.array([ES.best(v) for v in np.asarray(a, np.float32).reshape(-1)], np.int64).reshape(np.shape(a))


def best_fast(a):
    """The same on a vector at once (the two rounded differences, a tie goes up)."""
    a = np.asarray(a, np.float32)
    u = np.clip(np.searchsorted(KVF, a, side="right"), 1, 15)
    idx = np.where((a - KVF[u - 1]) < (KVF[u] - a), u - 1, u)
    return np.where(a <= KVF[0], 0, np.where(a >= KVF[15], 15, idx))


def loop_scales(t, panel, imp):
    """panel fp32 [R, 256], imp fp32 [256] or None -> (d bits uint16 [R, 1 or 8], ls int [R, 8] or None, step, istep fp32 [R, 8])
    by the loops of iq4_encode_spec."""
    R = panel.shape[0]
    size = 256 if t == XS else 32
    dbits = np.zeros((R, 256 // size), np.uint16)
    ls = np.zeros((R, 8), np.int64) if t == XS else None
    step, istep = np.zeros((R, 8), np.float32), np.zeros((R, 8), np.float32)
    with np.errstate(all="ignore"):
        for r in range(R):
            for sb in range(256 // size):
                x = panel[r, size * sb:size * sb + size]
                im = None if imp is None else imp[size * sb:size * sb + size]
                s = F(0)
                for j in range(size):
                    s = F(s + F(x[j] * x[j]))
                sigma2 = F(s * F(F(2) / F(size)))
                ds = []
                for ib in range(size // 32):
                    xb = x[32 * ib:32 * ib + 32]
                    use = im is not None and any(im[32 * ib + j] != 0 for j in range(32))
                    w = [F(im[32 * ib + j] * np.sqrt(F(sigma2 + F(xb[j] * xb[j])), dtype=np.float32)) if use else F(xb[j] * xb[j])
                         for j in range(32)]
                    ds.append(ES.block_scale(xb, w))
                if t == NL:
                    d = ds[0]
                    dbits[r, sb] = _f2h_bits(d)
                    step[r, sb] = _h2f(dbits[r, sb])
                    istep[r, sb] = F(F(1) / d) if d != 0 else F(0)
                    continue
                amax, ms = F(0), F(0)
                for d in ds:
                    if F(abs(d)) > amax:
                        amax, ms = F(abs(d)), d
                D = F(F(-ms) / F(32))
                iD = F(F(1) / D) if D != 0 else F(0)
                dbits[r, 0] = _f2h_bits(D)
                for ib in range(8):
                    l = int(max(-32, min(31, np.rint(F(iD * ds[ib])))))
                    dl = F(D * F(l))
                    ls[r, ib] = l + 32
                    step[r, ib] = F(_h2f(dbits[r, 0]) * F(l))
                    istep[r, ib] = F(F(1) / dl) if dl != 0 else F(0)
    return dbits, ls, step, istep


def host_scales(t, panel, imp):
    """The same outputs from gguf_writer.iq4_scales."""
    from gptq_gguf_toolkit_amd import gguf_writer
    R = panel.shape[0]
    head, inv = gguf_writer.iq4_scales(np.ascontiguousarray(panel, np.float32), t, imp)
    istep = np.asarray(inv, np.float32).reshape(R, 8)
    if t == NL:
        dbits = np.ascontiguousarray(head).view(np.uint16).reshape(R, 8)
        return dbits, None, _h2f(dbits), istep
    head = np.ascontiguousarray(head).reshape(R, 8)
    dbits = np.ascontiguousarray(head[:, :2]).view(np.uint16).reshape(R, 1)
    sh = head[:, 2].astype(np.int64) | (head[:, 3].astype(np.int64) << 8)
    ls = np.stack([((head[:, 4 + ib // 2] >> (4 * (ib % 2))) & 15) | (((sh >> (2 * ib)) & 3) << 4) for ib in range(8)], 1)
    step = (_h2f(dbits) * (ls - 32).astype(np.float32)).astype(np.float32)
    return dbits, ls, step, istep


def walk(W, U, t, block_size=128, importance=None, scales=host_scales, best=best_fast):
    """-> dict(W, qweight, d (uint16 bits), ls (uint8, XS only), step, istep) of gq_gptq_quantize_iq4 on (W, U)."""
    W = np.array(W, np.float32, copy=True)
    U = np.ascontiguousarray(U, np.float32)
    R, C = W.shape
    assert C % 256 == 0
    imp = None if importance is None else np.ascontiguousarray(importance, np.float32)
    B = C if block_size <= 0 or block_size > C else block_size
    nb = C // 32
    q = np.zeros((R, C), np.uint8)
    d = np.zeros((R, C // 256 if t == XS else nb), np.uint16)
    ls = np.zeros((R, nb), np.uint8) if t == XS else None
    step, istep = np.zeros((R, nb), np.float32), np.zeros((R, nb), np.float32)
    with np.errstate(all="ignore"):
        for c1 in range(0, C, B):
            c2 = min(c1 + B, C)
            wb = W[:, c1:c2].copy()
            Err = np.zeros((R, c2 - c1), np.float32)
            for i in range(c2 - c1):
                j = c1 + i
                if j % 256 == 0:  # the GLOBAL W, as it is in memory now
                    db, l, st, ist = scales(t, W[:, j:j + 256], None if imp is None else imp[j:j + 256])
                    g0 = j // 32
                    step[:, g0:g0 + 8], istep[:, g0:g0 + 8] = st, ist
                    if t == XS:
                        d[:, j // 256:j // 256 + 1], ls[:, g0:g0 + 8] = db, l
                    else:
                        d[:, g0:g0 + 8] = db
                w = wb[:, i].copy()
                code = best((istep[:, j // 32] * w).astype(np.float32))
                wq = (step[:, j // 32] * KVF[code]).astype(np.float32)
                q[:, j], W[:, j] = code, wq
                err = ((w - wq).astype(np.float32) / U[j, j]).astype(np.float32)
                Err[:, i] = err
                if i + 1 < c2 - c1:  # self + (alpha * err) * u: the product rounded, then the sum
                    prod = ((-err)[:, None] * U[j, j + 1:c2][None, :]).astype(np.float32)
                    wb[:, i + 1:] = (wb[:, i + 1:] + prod).astype(np.float32)
            if c2 < C:
                W[:, c2:] = trailing_update(W[:, c2:], Err, U[c1:c2, c2:])
    return dict(W=W, qweight=q, d=d, ls=ls, step=step, istep=istep)


def pack(t, out, row_src=None):
    """The walk's outputs as block bytes uint8 [R, row bytes] in the layouts of gptq_gguf_iq4.h."""
    q, d, ls = out["qweight"], out["d"], out["ls"]
    R, C = q.shape
    rows = range(R) if row_src is None else row_src
    res = bytearray()
    for r in rows:
        for sb in range(C // (256 if t == XS else 32)):
            if t == NL:
                L = q[r, 32 * sb:32 * sb + 32]
                res += struct.pack("<H", int(d[r, sb])) + bytes(int(L[k]) | (int(L[k + 16]) << 4) for k in range(16))
                continue
            l = [int(v) for v in ls[r, 8 * sb:8 * sb + 8]]
            scales_h = sum((l[ib] >> 4) << (2 * ib) for ib in range(8))
            scales_l = bytes((l[2 * k] & 15) | ((l[2 * k + 1] & 15) << 4) for k in range(4))
            res += struct.pack("<HH", int(d[r, sb]), scales_h) + scales_l
            for ib in range(8):
                L = q[r, 256 * sb + 32 * ib:256 * sb + 32 * ib + 32]
                res += bytes(int(L[k]) | (int(L[k + 16]) << 4) for k in range(16))
    return np.frombuffer(bytes(res), np.uint8).reshape(R, -1)


# ---------------------------------------------------------------------------------------------------------------- quality
def correlated_problem(rng, R, C, rank, eps):
    """W = 0.02 N(0, 1); X = Z_r A / sqrt(rank) + eps Z, scaled per channel by exp(0.5 N(0, 1)), T = 4C; H = 2 / T X^T X, damped
    by 1 % of mean(diag H).  -> (W fp32, H fp64 damped, diag of the undamped H fp32)"""
    T = 4 * C
    W = (0.02 * rng.standard_normal((R, C))).astype(np.float32)
    X = rng.standard_normal((T, rank)) @ rng.standard_normal((rank, C)) / np.sqrt(rank) + eps * rng.standard_normal((T, C))
    X = X * np.exp(0.5 * rng.standard_normal(C))
    H = 2.0 / T * (X.T @ X)
    diag = np.diag(H).astype(np.float32).copy()
    H = H + 0.01 * np.mean(np.diag(H)) * np.eye(C)
    return W, H, diag


def quality_problems():
    """The two correlated problems of the quality condition: default_rng seeds 1 and 2, drawn in this order."""
    return [correlated_problem(np.random.default_rng(1), 64, 512, 32, 0.3), correlated_problem(np.random.default_rng(2), 70, 768, 48, 0.1)]


def upper_factor(H):
    """U with U^T U = H^-1, upper triangular (gptq.py: cholesky of the inverse, upper), fp32."""
    Hinv = np.linalg.inv(H)
    return np.ascontiguousarray(np.linalg.cholesky(Hinv).T, np.float32)


def relative_error(W0, Wq, H):
    """sum(dW H o dW) / sum(W H o W) in fp64"""
    dW, W0 = np.asarray(Wq, np.float64) - np.asarray(W0, np.float64), np.asarray(W0, np.float64)
    return float(np.sum((dW @ H) * dW) / np.sum((W0 @ H) * W0))
