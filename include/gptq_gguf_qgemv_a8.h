/* gptq_gguf_qgemv_a8.h -- the packed-weight decode step on int8 activations: gq_gemv_packed's call with gq_linear_packed_a8's
   arithmetic.  One launch quantizes the few tokens of x to the Q8 activation format of gptq_gguf_qgemm_a8.h (inside the
   kernel, into LDS) and multiplies the integer codes of the packed weight with them on the VALU's 4 x int8 dot product.
   An additive extension of the C ABI of gptq_gguf.h (same library, same conventions: status codes, gq_last_error,
   GQ_F16 / GQ_BF16, device pointers, `stream` a hipStream_t).  GQ_ABI_VERSION does not change.  Every check is made before the
   first HIP call: a refused call has launched nothing. */
#ifndef GPTQ_GGUF_QGEMV_A8_H
#define GPTQ_GGUF_QGEMV_A8_H

#include "gptq_gguf_qgemm_a8.h"
#include "gptq_gguf_qgemv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_GEMV_A8_MAX_T 4 /* the most tokens of one gq_gemv_packed_a8 call */

/* ---- y[t, r] = round_once_to_x_dtype( sum_j term_j(t, r) ),  t = 0 .. T - 1,  r = 0 .. R - 1,  1 <= T <= GQ_GEMV_A8_MAX_T.
   Every argument is gq_gemv_packed's and means the same (blocks, row_src, R, C, x contiguous [T, C], y contiguous [T, R] in
   x_dtype, alignments), with two differences:
     T       T < 1 or T > GQ_GEMV_A8_MAX_T is GQ_E_BAD_SHAPE (gq_last_error gives T=<value>); gq_gemv_packed takes up to 16.
     q_type  GQ_Q2_K .. GQ_Q6_K or GQ_Q8_0.  GQ_IQ4_NL and GQ_IQ4_XS are NOT served: GQ_E_BAD_TYPE, the message names the type.
   and one more refusal: the quantized image of x lives in LDS, T * C * 73 / 64 bytes of it (gq_gemv_a8_plan); a (T, C) whose
   image does not fit is GQ_E_BAD_SHAPE and the message names T and C.  T = 4 fits up to C = 28672.
   Checks in gq_gemv_packed's order: q_type, x_dtype; NULL (blocks, x, y); R; T; C; the image; alignments (blocks, row_src, x, y).

   Nothing outside the blocks' extent, [x, x + T * C * 2) and [y, y + T * R * 2) is read or written.  The 2-byte aligned types
   are fetched with aligned 4-byte loads and a byte shift; where a 4-byte window would begin before a piece of a block or end
   after it, that end is a 2-byte load, so the loads cover exactly the blocks' bytes.

   Numerics.  (xq, xd, xbsum) are, byte for byte, what gq_quantize_act_q8 writes for x (gptq_gguf_qgemm_a8.h states every
   operation), and term_j is gq_linear_packed_a8's: for a K-quant block j of row r
     isum_j = sum_g sc_g * sum_{k in g} w_k * xq_k,   msum_j = sum_g mn_g * xbsum_g          exact in int32
     term_j = xd[t, j] * (d * float(isum_j) - dmin * float(msum_j))                          in fp32, each operation rounded once
   (Q3_K, Q6_K: term_j = xd[t, j] * (d * float(isum_j))), and for GQ_Q8_0, with the eight blocks b of superblock j,
     term_j = xd[t, j] * (sum_b d_b * float(isum_b)),  the sum over b in fp32 as ((b0 + b1) + (b2 + b3)) + ((b4 + b5) + (b6 + b7)).
   The terms are added in fp32 in a fixed order that is NOT gq_linear_packed_a8's: partial sums s_i = term_i + term_{i+16} +
   term_{i+32} + .. (ascending) for i = 0 .. 15, then a binary tree over i (distance 1, 2, 4, 8).  One rounding (nearest even)
   to x_dtype.  So the result differs from gq_linear_packed_a8's on the same x by fp32 summation order only, and both lie
   within the same bound of the exact sum.  The weight is never rounded to 16 bits.
   Deterministic: a wave owns whole rows, no split of C across waves or workgroups, no atomics; a row's result depends on its
   row and on x only, not on R or on the row's place in the grid.  The call only enqueues: one launch, no workspace, no
   allocation, no host synchronisation. */
int gq_gemv_packed_a8(int q_type, const void* blocks, const int32_t* row_src, int64_t R, int64_t C,
                      const void* x, int64_t T, int x_dtype, void* y, void* stream);

/* ---- how gq_gemv_packed_a8 would run (T, R, C), without a device: lds_bytes of the image, rows_per_turn a workgroup takes
   per turn of its grid-stride loop, grid_cap, grid = min(ceil(R / rows_per_turn), grid_cap) and fits (1 / 0: the image is
   within the LDS budget).  Any output pointer may be NULL.  T < 1, T > GQ_GEMV_A8_MAX_T, R out of [1, 2^31) or C % 256 != 0:
   GQ_E_BAD_SHAPE. */
int gq_gemv_a8_plan(int64_t T, int64_t R, int64_t C, int64_t* lds_bytes, int64_t* rows_per_turn, int64_t* grid_cap,
                    int64_t* grid, int64_t* fits);

#ifdef __cplusplus
}
#endif
#endif
