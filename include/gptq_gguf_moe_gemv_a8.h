/* gptq_gguf_moe_gemv_a8.h -- the decode step of a packed mixture-of-experts layer on int8 activations: gq_gemv_packed_experts'
   call (gptq_gguf_moe.h) with gq_gemv_packed_a8's arithmetic (gptq_gguf_qgemv_a8.h).  One launch quantizes the input rows of
   the step's (token, expert) pairs to the Q8 activation format of gptq_gguf_qgemm_a8.h (inside the kernel, into LDS; with
   x_up, SwiGLU first) and multiplies the integer codes of each pair's expert with them on the VALU's 4 x int8 dot product.
   An additive extension of the C ABI of gptq_gguf.h (same library, same conventions: status codes, gq_last_error,
   GQ_F16 / GQ_BF16, device pointers, `stream` a hipStream_t).  GQ_ABI_VERSION does not change.  Every check is made before the
   first HIP call: a refused call has launched nothing. */
#ifndef GPTQ_GGUF_MOE_GEMV_A8_H
#define GPTQ_GGUF_MOE_GEMV_A8_H

#include "gptq_gguf_moe.h"
#include "gptq_gguf_qgemv_a8.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- y[p, r] = round_once_to_x_dtype( sum_j term_j(p, r) ),  p = 0 .. P - 1 with 0 <= pair_expert[p] < E,  r = 0 .. R - 1.
   Every argument but x_up is gq_gemv_packed_experts' and means the same: blocks the stacked [E, R, C] tensor, expert-major, at
   the block's natural alignment; x contiguous [x_rows, C]; pair_expert P int32 ON THE DEVICE, never read by the host; pair p
   takes row p / pairs_per_row of x and writes row p of y (contiguous [P, R]); x_rows * pairs_per_row == P,
   1 <= P <= GQ_MOE_MAX_PAIRS, 1 <= E <= 65535.  A pair_expert value outside [0, E) is not checked and is no error: that pair
   is skipped and its row of y is not written.  The weight bytes of an expert that no pair names are not read.  Differences:
     q_type  GQ_Q2_K .. GQ_Q6_K or GQ_Q8_0.  GQ_IQ4_NL and GQ_IQ4_XS are NOT served: GQ_E_BAD_TYPE, the message names the type.
     x_up    NULL, or a second contiguous [x_rows, C] tensor of x_dtype, 16-byte aligned: the input of pair p is then
             h = round16(round16(silu(x)) * x_up) of its row, element by element gq_fwd_silu_mul's operations (silu
             g / (1 + exp(-g)) in fp32, rounded to x_dtype, times up, rounded to x_dtype), and h is never written to memory.
             Meant for the down projection (pairs_per_row = 1, x the gate and x_up the up result).
     image   the quantized rows of a pass -- at most 4 matching pairs of one expert -- live in LDS, min(P, 4) * C * 73 / 64
             bytes (gq_gemv_experts_a8_plan); a (P, C) whose image does not fit is GQ_E_BAD_SHAPE and the message names P, C
             and both byte counts.  P >= 4 fits up to C = 28672.
   Checks in this order: q_type, x_dtype; NULL (blocks, x, pair_expert, y); E; R; P; x_rows * pairs_per_row; C; the image;
   alignments (blocks, pair_expert 4, x 16, x_up 16, y 16).

   Nothing outside the blocks' extent, [x, x + x_rows * C * 2) (and the same extent of x_up), pair_expert[0 .. P) and
   [y, y + P * R * 2) is read or written; the 2-byte aligned types are fetched as gq_gemv_packed_a8 fetches them, with loads
   that cover exactly the blocks' bytes.

   Numerics.  The image of a pair's input row is, byte for byte, what gq_quantize_act_q8 writes for that row (x_up:
   what gq_silu_mul_quantize_act_q8(x, x_up) writes, gptq_gguf_moe_gemm_a8.h), and term_j and the order of the fp32 additions
   are gq_gemv_packed_a8's (gptq_gguf_qgemv_a8.h states every operation): partial sums s_i = term_i + term_{i+16} + .. for
   i = 0 .. 15, a binary tree over i, one rounding (nearest even) to x_dtype.  The two kernels run one text, so row p of y
   is, BIT FOR BIT, what gq_gemv_packed_a8 writes for (q_type, blocks + pair_expert[p] * expert bytes, row_src = NULL, R, C,
   x + (p / pairs_per_row) * C elements, T = 1, x_dtype) -- with x_up: for the row h written by gq_fwd_silu_mul.  The result
   of a pair does not depend on which other pairs the call holds, on P, on the order of the pairs or on the pass it falls
   into (an expert named by more than 4 pairs takes further passes of 4 over its weight).
   Deterministic: a wave owns whole rows, no split of C across waves or workgroups, no atomics.  The call only enqueues: one
   launch of a grid (grid_x, E), no workspace, no allocation, no host synchronisation. */
int gq_gemv_packed_experts_a8(int q_type, const void* blocks, int64_t E, int64_t R, int64_t C,
                              const void* x, const void* x_up, int64_t x_rows, const int32_t* pair_expert, int64_t P,
                              int64_t pairs_per_row, int x_dtype, void* y, void* stream);

/* ---- how gq_gemv_packed_experts_a8 would run (P, R, C), without a device: lds_bytes of the image of min(P, 4) rows,
   rows_per_turn a workgroup takes per turn of its grid-stride loop over an expert's rows, grid_x_cap, grid_x =
   min(ceil(R / rows_per_turn), grid_x_cap) (the launch's grid is (grid_x, E)) and fits (1 / 0: the image is within the LDS
   budget).  Any output pointer may be NULL.  P out of [1, GQ_MOE_MAX_PAIRS], R out of [1, 2^31) or C % 256 != 0:
   GQ_E_BAD_SHAPE. */
int gq_gemv_experts_a8_plan(int64_t P, int64_t R, int64_t C, int64_t* lds_bytes, int64_t* rows_per_turn,
                            int64_t* grid_x_cap, int64_t* grid_x, int64_t* fits);

#ifdef __cplusplus
}
#endif
#endif
