/* gptq_gguf_moe_calib.h -- the calibration forward of a mixture-of-experts layer whose experts are dense 16-bit weights
   (transformers' fused MixtralExperts): the last step, the weighted sum of the experts' outputs per token, in one launch
   with the roundings of transformers' eager loop.  An additive extension of the C ABI of gptq_gguf.h in the way of
   gptq_gguf_moe_gemm.h (same library, same conventions: status codes, gq_last_error, GQ_F32 / GQ_F16 / GQ_BF16, device
   pointers, `stream` a hipStream_t).  GQ_ABI_VERSION does not change. */
#ifndef GPTQ_GGUF_MOE_CALIB_H
#define GPTQ_GGUF_MOE_CALIB_H

#include "gptq_gguf_moe_gemm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_MOE_COMBINE_MAX_K 8 /* the most experts per token */

/* ---- out[t] = the sum over token t's experts of w[t, k] * y[row of pair (t, k)], rounded the way transformers'
   MixtralExperts.forward rounds it: per hit expert, in ascending expert id,
       h = y_e * w[token_idx, top_k_pos, None];  final.index_add_(0, token_idx, h.to(final.dtype))
   into final = zeros_like(hidden_states).

   The pairs are numbered p = k * T + t (the router's [T, K] index TRANSPOSED, then flattened): gq_moe_route's stable sort of
   these pairs yields, inside every expert's run, the row order of transformers' torch.where(expert_mask[e]) -- by choice k,
   then by token.
   y: [P, H] contiguous, P = T * K, fp16 or bf16 (`dtype`): the down-projection outputs in EXPERT-SORTED order; row s belongs
   to pair order[s].  Only the rows s < expert_start[E] are read.
   pair_expert (P int32), expert_start (E + 1 int32), order (P int32): what gq_moe_route was given and wrote for this P and E,
   on the device, never read by the host.
   w: [T, K] contiguous, GQ_F32 or `dtype` (`w_dtype`).
   out: [T, H] contiguous, `dtype`.  Every element is written.

   Contract (exact), per token t and element h:
       acc = +0
       for the token's valid pairs in ascending expert id, ties (one token naming an expert twice) by k ascending:
           v   = round_dtype(float(y[s, h]) * float(w[t, k]))      -- the fp32 product, then one rounding to `dtype`
           acc = round_dtype(float(acc) + float(v))                -- the fp32 sum, then one rounding to `dtype`
       out[t, h] = acc
   A pair whose id lies outside [0, E) contributes nothing (transformers uses E for a masked pair); a token without a valid
   pair gets +0.  The first product is ADDED to +0, not stored: a -0 product gives +0, as zeros_like + index_add_ does.  The
   rounding of v sits between the multiply and the add: there is nothing to contract.  (For a token that names no expert twice
   this is transformers' result bit for bit: one index_add_ per expert adds at most one row to the token.)

   No inverse of `order` is needed and no workspace: the position s of pair p is found by a binary search for p in its
   expert's run order[expert_start[e] .. expert_start[e + 1]), which gq_moe_route leaves ascending -- K searches of at most
   17 steps per token, by K lanes side by side, next to K * H values read.  A pair that is not found in its run (an `order`
   that is not this pair_expert's) contributes nothing; a run is clamped to [0, P].

   1 <= K <= GQ_MOE_COMBINE_MAX_K, 1 <= E <= GQ_MOE_ROUTE_MAX_EXPERTS, T >= 1 and T * K <= GQ_MOE_ROUTE_MAX_PAIRS, H >= 8 and
   H % 8 == 0; y and out 16-byte aligned, the int32 arrays 4-byte aligned, w aligned to its element.
   Status codes as gq_moe_route's; the checks run in the order dtype, w_dtype, NULL pointers, E, K, T, H, alignments and
   gq_last_error names the offending value (dtype, w_dtype, E=, K=, T=, H=).  Every check is made before the first HIP call:
   a refused call has launched nothing.

   ONE launch: a workgroup per token (the grid capped at 2048 workgroups, the tokens strided over it); the token's K entries
   are sorted in registers by wave 0; every lane then reads K times 16 bytes of y and writes 16 bytes of out per 8 elements.
   Deterministic: no atomics.  Nothing outside [y, y + P * H * 2), pair_expert[0 .. P), expert_start[0 .. E], order[0 .. P),
   w[0 .. T * K) and [out, out + T * H * 2) is read or written.  The call only enqueues: no allocation, no host
   synchronisation. */
int gq_fwd_moe_combine(const void* y, const int32_t* pair_expert, const int32_t* expert_start, const int32_t* order,
                       const void* w, int w_dtype, int64_t T, int64_t K, int64_t E, int64_t H, int dtype, void* out,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
