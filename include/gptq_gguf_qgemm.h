/* gptq_gguf_qgemm.h -- the packed-weight forward: a Linear whose weight exists only as GGUF block bytes (K-quants, Q8_0).
   An additive extension of the C ABI of gptq_gguf.h (same library, same conventions: status codes, gq_last_error,
   GQ_F16 / GQ_BF16, device pointers, `stream` a hipStream_t).  GQ_ABI_VERSION does not change.  The symbol lives in a
   header of its own so that gptq_gguf.h stays the symbol set its version names. */
#ifndef GPTQ_GGUF_QGEMM_H
#define GPTQ_GGUF_QGEMM_H

#include "gptq_gguf_q8.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- y[t, r] = sum_c x[t, c] * w[r, c],   t = 0 .. T - 1,   r = 0 .. R - 1,   for a weight [R, C] given as packed blocks:
   w[r, :] = decode(blocks row (row_src ? row_src[r] : r)).  No dense [R, C] weight exists before, during or after the call.

     q_type  GQ_Q2_K .. GQ_Q6_K or GQ_Q8_0 (with gptq_gguf_iq4.h also GQ_IQ4_NL and GQ_IQ4_XS, under the rules stated there);
             anything else is GQ_E_BAD_TYPE.
     blocks  R rows of C / 256 blocks (Q8_0: C / 32 blocks of 34 bytes), as gq_level_switch takes them for the same kind:
             aligned to the block's natural alignment (Q2_K 4 bytes, Q3_K / Q6_K / Q8_0 2, Q4_K / Q5_K 16).  Staging loads
             are that wide and cover exactly the blocks' bytes: nothing outside [blocks, blocks + R * C / 256 * type_size)
             (Q8_0: R * C / 32 * 34) is read.
     row_src NULL (identity) or R int32 row indices on the device, 4-byte aligned, each in [0, R) -- the kernel does not check.
     C % 256 == 0 for EVERY kind, Q8_0 included (the K-step is one 256-value superblock); 256 <= C < 2^31.  R >= 1, T >= 1,
             T < 2^31 and R < 2^31.
     x       contiguous [T, C] in x_dtype GQ_F16 or GQ_BF16 (GQ_F32 and anything else: GQ_E_BAD_TYPE), 16-byte aligned.
     y       contiguous [T, R] in the same dtype, 16-byte aligned.  Nothing outside [y, y + T * R * 2) is written.
   GQ_E_BAD_SHAPE for the shape rules and alignments, GQ_E_NULL for blocks / x / y; gq_last_error names the argument.  Every
   check is made before the first HIP call: a refused call has launched nothing (and host pointers can be refused on a
   machine without a GPU).

   Numerics.  The weight operand is, bit for bit, what gq_dequantize_blocks writes for (q_type, blocks, R, C, row_src,
   out_dtype = x_dtype): the fp32 decode rounded ONCE to the 16-bit type -- exactly the live weight a dense gq_level_switch
   produces.  It is decoded in registers by the same device functions as there.  Products of two 16-bit operands are exact
   in fp32; accumulation is fp32 in the matrix pipe, in an order this header does not promise; the sum is rounded once
   (nearest-even) to x_dtype.  So the result differs from a GEMM on the decoded weight only by fp32 summation order.
   Deterministic: one workgroup owns an output tile and walks all of C, no split-K across workgroups, no atomics -- the same
   call gives the same bits.
   The call only enqueues: no workspace, no allocation, no host synchronisation. */
int gq_linear_packed(int q_type, const void* blocks, const int32_t* row_src, int64_t R, int64_t C,
                     const void* x, int64_t T, int x_dtype, void* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif
