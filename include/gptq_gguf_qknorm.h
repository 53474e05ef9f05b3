/* gptq_gguf_qknorm.h -- the part of the calibration forward that Qwen3 adds to a Llama decoder layer: the per-head RMSNorm
   over head_dim on q and k (q_norm, k_norm) and the rotary embedding that follows, for BOTH tensors in one launch, with the
   roundings and the summation order of transformers' eager ops.  An additive extension of the C ABI of gptq_gguf.h in the way
   of gptq_gguf_moe_calib.h (same library, same conventions: status codes, gq_last_error, GQ_F16 / GQ_BF16, device pointers,
   `stream` a hipStream_t).  GQ_ABI_VERSION does not change. */
#ifndef GPTQ_GGUF_QKNORM_H
#define GPTQ_GGUF_QKNORM_H

#include "gptq_gguf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Qwen3RMSNorm.forward over head_dim, then apply_rotary_pos_emb, on q and k.

   q [tokens, heads_q, head_dim], k [tokens, heads_k, head_dim]: the projections' own layout (q_proj(x).view(B, L, H, D)),
   contiguous, `dtype` (GQ_F16 or GQ_BF16).  wq, wk: [head_dim] in `dtype` (q_norm.weight, k_norm.weight).  cos_, sin_:
   [tokens, head_dim] in `dtype`.  q_out, k_out: the layouts of q and k; they do not overlap any input.  head_dim is 64, 128
   or 256; 1 <= heads_q, heads_k; tokens >= 1.  Every pointer is 16-byte aligned.
   stats: NULL, or fp32 [tokens * (heads_q + heads_k), 2], 4-byte aligned, the q rows (token-major, then head) first, then
   the k rows: each row's `var` and `r` below as the kernel computed them (16-bit outputs hide most differences of the
   summation order; the caller that wants to TRUST the kernel compares these with torch's own mean and rsqrt).

   Contract (exact) per (token, head) row x[0 .. D), D = head_dim, every product and sum in fp32 without contraction:
       s   = the sum of float(x[d])^2 in the order of ATen's reduce kernel for mean(-1) of a contiguous fp32 [rows, D] tensor on
             a 64-wide wavefront (aten/src/ATen/native/cuda/Reduce.cuh: setReduceConfig vectorises from 128 values per output
             on and block_width stays within the wavefront.  MEASURED on an MI355X, profiles/qk_norm_order_probe.py and
             DESIGN.md K32: var and r equal torch's in every row at 2 .. 81920 rows -- the order does NOT depend on the
             number of rows --, and D = 64 is NOT the 4-accumulator form of the wider rows):
               D = 64:         64 leaves p[j] = x[j]^2                                        (no vectorised load: D < 128)
               D = 128, 256:   D / 4 leaves p[j] = ((x[4j]^2 + x[4j+1]^2) + x[4j+2]^2) + x[4j+3]^2   (one 4-element vector
                               per lane, four accumulators folded in index order)
             and the leaves summed as a balanced binary tree in index order (shuffle-down offsets 1, 2, 4, ... over the
             row's lanes: (p[0] + p[1]) + (p[2] + p[3]), ...);
       var = s * (1 / D)                    -- ATen's factor float(outputs) / inputs, exact for these D
       r   = 1 / sqrt(var + eps), correctly rounded to fp32 (torch.rsqrt on this stack)
       y   = round_dtype(float(x[d]) * r)
       z   = round_dtype(float(w[d]) * y)
       out[d]       = round_dtype(round_dtype(z[d] * cos[d])             + round_dtype(-z[d + D/2] * sin[d]))         d <  D/2
       out[d + D/2] = round_dtype(round_dtype(z[d + D/2] * cos[d + D/2]) + round_dtype(z[d] * sin[d + D/2]))
   -- gq_fwd_rope's per-op rounding.  Nothing is free-order: the result is bit-identical to the eager ops or the caller
   does not use it (forward_fused.py verifies on the first input of every shape class).

   Status: GQ_E_BAD_TYPE (dtype not GQ_F16 / GQ_BF16), GQ_E_NULL (a NULL pointer other than stats), GQ_E_BAD_SHAPE
   (head_dim not 64 / 128 / 256, tokens < 1, heads < 1, a pointer that is not 16-byte aligned, more rows than one grid
   takes: tokens * ceil((heads_q + heads_k) / 4) * head_dim / 16 lanes must fit 2^31 - 1 workgroups of 256), checked in that
   order before the first HIP call: a refused call has launched nothing.

   ONE launch, no grid cap and no loop: head_dim / 16 lanes own up to four consecutive heads of one token (q heads first,
   then k heads), so a wavefront holds 16 .. 64 rows; a lane keeps its 16 elements of every row in registers from the two
   16-byte loads to the two 16-byte stores, and loads the token's cos / sin once for its rows.  HBM traffic: one read and one
   write of q and k, cos / sin once per four heads (from cache after the first).  No workspace, no atomics, no host
   synchronisation; deterministic.  Nothing outside the tensors named above is read or written. */
int gq_fwd_qk_norm_rope(const void* q, const void* k, const void* wq, const void* wk, const void* cos_, const void* sin_,
                        void* q_out, void* k_out, int64_t tokens, int heads_q, int heads_k, int head_dim, float eps, int dtype,
                        float* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
