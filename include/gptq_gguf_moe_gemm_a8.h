/* gptq_gguf_moe_gemm_a8.h -- the packed MoE prefill on int8 activations: the grouped expert GEMM on the int8 matrix pipe and
   the SwiGLU that writes its result as quantized activations.  An additive extension of the C ABI of gptq_gguf.h in the way
   of gptq_gguf_moe_gemm.h and gptq_gguf_qgemm_a8.h (same library, same conventions: status codes, gq_last_error, GQ_F16 /
   GQ_BF16, device pointers, `stream` a hipStream_t).  GQ_ABI_VERSION does not change.  Every check is made before the first
   HIP call and names its argument: a refused call has launched nothing (and host pointers can be refused on a machine without
   a GPU). */
#ifndef GPTQ_GGUF_MOE_GEMM_A8_H
#define GPTQ_GGUF_MOE_GEMM_A8_H

#include "gptq_gguf_moe_gemm.h"
#include "gptq_gguf_qgemm_a8.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- for every pair p in order[0 .. expert_start[E]):   y[p, :] = W[e] (xq, xd, xbsum)[p / pairs_per_row],
   e the expert whose run [expert_start[e], expert_start[e + 1]) holds p: gq_linear_packed_experts with the activations and
   the arithmetic of gq_linear_packed_a8.

     blocks   the stacked [E, R, C] tensor as GGUF block bytes, as for gq_linear_packed_experts.
     q_type   GQ_Q2_K .. GQ_Q6_K or GQ_Q8_0.  GQ_IQ4_NL and GQ_IQ4_XS are NOT served: GQ_E_BAD_TYPE, the message names the
              type; anything else is GQ_E_BAD_TYPE as well.  All six served types are built (none had to be left out for its
              registers).
     xq, xd, xbsum   gq_quantize_act_q8's (or gq_silu_mul_quantize_act_q8's) outputs for x_rows rows of C values,
              x_rows * pairs_per_row == P; 16-byte aligned.
     expert_start, order   gq_moe_route's outputs for the same P and E, ON THE DEVICE, never read by the host; trusted as
              gq_linear_packed_experts trusts them (an entry of `order` outside [0, P) is skipped, as -1 is).
     y        contiguous [P, R] of y_dtype (GQ_F16 or GQ_BF16, else GQ_E_BAD_TYPE), 16-byte aligned.
   1 <= E <= GQ_MOE_ROUTE_MAX_EXPERTS, 1 <= P <= GQ_MOE_ROUTE_MAX_PAIRS, 1 <= R < 2^31, C % 256 == 0, 256 <= C < 2^31.
   Checks in this order: q_type, y_dtype; NULL (blocks, xq, xd, xbsum, expert_start, order, y); E; R; P; x_rows *
   pairs_per_row; C; alignments (blocks, expert_start, order, xq, xd, xbsum, y).

   Numerics: row p of y is, BIT FOR BIT, what gq_linear_packed_a8 writes for (q_type, blocks + e * expert bytes, row_src =
   NULL, R, C) and the quantized row p / pairs_per_row: the two kernels run one text (csrc/qgemm/gq_qgemm_a8_core.hpp), in which
   an output element is an exact integer part per superblock and a fixed fp32 sequence in ascending superblock order, whatever
   the token's place in the tile and the other tokens are.  So the result of a pair does not depend on which other pairs the
   call holds, on P or on the routing.

   A pair in no run of the route is skipped and its row of y is NOT written.  The weight bytes of an expert with an empty run
   are not read.  Nothing outside the blocks' extent, the three activation tensors' x_rows rows, expert_start[0 .. E],
   order[0 .. P) and [y, y + P * R * 2) is read or written.

   ONE launch of ceil(R / 128) x (ceil(P / 128) + min(E, P)) workgroups (gq_linear_packed_experts' bound for 128-token tiles;
   there is no wider tile); a workgroup without work returns before any staging, and a tile's empty 32-token quarters cost no
   matrix instruction.  Deterministic: no atomics, no split across workgroups.  The call only enqueues: no workspace, no
   allocation, no host synchronisation. */
int gq_linear_packed_experts_a8(int q_type, const void* blocks, int64_t E, int64_t R, int64_t C,
                                const int8_t* xq, const float* xd, const int16_t* xbsum, int64_t x_rows,
                                int64_t pairs_per_row, const int32_t* expert_start, const int32_t* order,
                                int64_t P, void* y, int y_dtype, void* stream);

/* ---- (gate, up) [P, I] -> (xq, xd, xbsum) of  h = silu(gate) * up,  BYTE FOR BYTE gq_quantize_act_q8(gq_fwd_silu_mul(gate,
   up)) without h ever being written: per element, in fp32 on the inputs widened exactly,
     s = round_to_dtype(g / (1 + expf(-g)));   h = round_to_dtype(s * u)
   (the two roundings of gq_fwd_silu_mul), then gq_quantize_act_q8's rule on the 256 values of h of a superblock (amax, inv,
   rint, d; a NaN is skipped by amax and gets code 0, an infinity makes d = +inf and every code 0).
   gate, up contiguous of dtype GQ_F16 or GQ_BF16 (else GQ_E_BAD_TYPE); I % 256 == 0, 256 <= I < 2^31, 1 <= P < 2^31 and
   P * I / 2048 < 2^31 (GQ_E_BAD_SHAPE); the five pointers non-NULL (GQ_E_NULL) and 16-byte aligned (GQ_E_BAD_SHAPE).
   Checks in this order: dtype, NULL (gate, up, xq, xd, xbsum), P, I, the product, alignments (same order).
   One launch, no LDS, no workspace, no atomics; the same call gives the same bytes. */
int gq_silu_mul_quantize_act_q8(const void* gate, const void* up, int64_t P, int64_t I, int dtype,
                                int8_t* xq, float* xd, int16_t* xbsum, void* stream);

#ifdef __cplusplus
}
#endif
#endif
