/* gptq_gguf_qgemv.h -- the packed-weight forward for a few tokens: the decode step of a model whose Linear weights exist only
   as GGUF block bytes (K-quants, Q8_0).  An additive extension of the C ABI of gptq_gguf.h in the way of gptq_gguf_qgemm.h
   (same library, same conventions: status codes, gq_last_error, GQ_F16 / GQ_BF16, device pointers, `stream` a hipStream_t).
   GQ_ABI_VERSION does not change. */
#ifndef GPTQ_GGUF_QGEMV_H
#define GPTQ_GGUF_QGEMV_H

#include "gptq_gguf_qgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_GEMV_MAX_T 16 /* the most tokens of one gq_gemv_packed call */

/* ---- y[t, r] = sum_c x[t, c] * w[r, c],   t = 0 .. T - 1,   r = 0 .. R - 1,   1 <= T <= GQ_GEMV_MAX_T: gq_linear_packed for
   the few tokens of a decode step.  Every argument is gq_linear_packed's and means the same -- q_type GQ_Q2_K .. GQ_Q6_K or
   GQ_Q8_0; blocks R rows of C / 256 blocks (Q8_0: C / 32 of 34 bytes) at the block's natural alignment (Q2_K 4 bytes, Q3_K /
   Q6_K / Q8_0 2, Q4_K / Q5_K 16); row_src NULL or R int32 on the device, each in [0, R) (not checked by the kernel);
   C % 256 == 0 for every kind, 256 <= C < 2^31; 1 <= R < 2^31; x contiguous [T, C] and y contiguous [T, R] in x_dtype GQ_F16
   or GQ_BF16, both 16-byte aligned -- except T: T < 1 or T > GQ_GEMV_MAX_T is GQ_E_BAD_SHAPE (gq_last_error gives T=<value>);
   gq_linear_packed takes any number of tokens.  The status codes and the order of the checks are gq_linear_packed's, and
   every check is made before the first HIP call: a refused call has launched nothing.

   Nothing outside the blocks' extent (loads of the type's natural width that cover exactly the blocks' bytes), [x, x + T * C * 2)
   and [y, y + T * R * 2) is read or written; rows of y are R elements long, so for R % 4 != 0 the stores are 2 bytes wide.

   Numerics: gq_linear_packed's.  The weight operand is, bit for bit, what gq_dequantize_blocks writes for (q_type, blocks, R,
   C, row_src, out_dtype = x_dtype) -- the fp32 decode rounded ONCE to the 16-bit type, by the same device functions.  Products
   of two 16-bit operands are exact in fp32; accumulation is fp32, in a summation order this header does not promise (and
   which is not gq_linear_packed's); the sum is rounded once (nearest-even) to x_dtype.  So a packed model is one model at every
   T: the two calls differ by fp32 summation order only.
   Deterministic: one workgroup owns 16 rows and all of C; K is split across the waves of that workgroup only and their
   partial sums are added in a fixed wave order -- no split across workgroups, no atomics.  The same call gives the same bits.
   The call only enqueues: no workspace, no allocation, no host synchronisation. */
int gq_gemv_packed(int q_type, const void* blocks, const int32_t* row_src, int64_t R, int64_t C,
                   const void* x, int64_t T, int x_dtype, void* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif
