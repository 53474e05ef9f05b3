/* gptq_gguf_qgemm_a8.h -- the packed-weight forward on int8 activations: an activation quantizer (blocks of 256 values, modelled
   on ggml's Q8_K) and a GEMM that multiplies the integer codes of the packed weight with them on the int8 matrix pipe.
   An additive extension of the C ABI of gptq_gguf.h (same library, same conventions: status codes, gq_last_error,
   GQ_F16 / GQ_BF16, device pointers, `stream` a hipStream_t).  GQ_ABI_VERSION does not change.  Every check is made before the
   first HIP call: a refused call has launched nothing (and host pointers can be refused on a machine without a GPU).
   The format is modelled on ggml's block_q8_K; no bit-for-bit claim about llama.cpp is made. */
#ifndef GPTQ_GGUF_QGEMM_A8_H
#define GPTQ_GGUF_QGEMM_A8_H

#include "gptq_gguf_qgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- x [T, C] -> (xq, xd, xbsum).  A superblock is 256 consecutive values of one token; superblock j of token t:
     xq    int8  [T, C]        the codes
     xd    fp32  [T, C / 256]  the step
     xbsum int16 [T, C / 16]   xbsum[t, g] = the exact sum of the 16 codes xq[t, 16 g .. 16 g + 15]  (|sum| <= 2032)
   The arithmetic, every operation in fp32 (IEEE, round to nearest even) on the input widened exactly to fp32:
     amax = max |x| over the superblock (a NaN element is skipped)
     inv  = 127 / amax                              one division
     q    = clamp(rint(x * inv), -127, 127)         one multiply, ties to even
     d    = amax / 127                              one division
     amax == 0:  d = 0 and every q = 0.
   The author's rules for what the above leaves open:
     * amax so small that inv is not finite (amax < 127 / FLT_MAX, about 3.7e-37; bf16 inputs only): the superblock counts as
       zero, d = 0 and every q = 0.
     * a NaN element is skipped by amax and gets q = 0.  An infinite element makes amax = +inf, so inv = 0, every q = 0 and
       d = +inf: the outputs of that token are not finite downstream (inf * 0), which is how the input's defect is passed on.
   x is contiguous, x_dtype GQ_F16 or GQ_BF16 (else GQ_E_BAD_TYPE), C % 256 == 0, 256 <= C < 2^31, 1 <= T < 2^31 and
   T * C / 2048 < 2^31 (GQ_E_BAD_SHAPE); x, xq, xd, xbsum non-NULL (GQ_E_NULL) and 16-byte aligned (GQ_E_BAD_SHAPE).
   Checks in this order: x_dtype, NULL (x, xq, xd, xbsum), T, C, the product, alignments (same order).
   One launch, no workspace, no atomics; the same call gives the same bytes. */
int gq_quantize_act_q8(const void* x, int64_t T, int64_t C, int x_dtype, int8_t* xq, float* xd, int16_t* xbsum, void* stream);

/* ---- y[t, r] = round_once_to_y_dtype( sum_j term_j ),  j = 0 .. C / 256 - 1, for the packed weight [R, C] of
   gq_linear_packed (blocks, row_src, R, C: its rules, alignments and extents) and activations (xq, xd, xbsum) as above.

     q_type  GQ_Q2_K .. GQ_Q6_K or GQ_Q8_0.  GQ_IQ4_NL and GQ_IQ4_XS are NOT served: GQ_E_BAD_TYPE, the message names the
             type; anything else is GQ_E_BAD_TYPE as well.
     y_dtype GQ_F16 or GQ_BF16 (else GQ_E_BAD_TYPE).  y contiguous [T, R], 16-byte aligned; nothing outside
             [y, y + T * R * 2) is written.
     xq, xd, xbsum 16-byte aligned; xbsum must be the group sums of xq (the kernel uses it for the mins and does not check).
   Checks in gq_linear_packed's order: q_type, y_dtype; NULL (blocks, xq, xd, xbsum, y); R; T; C; alignments (blocks, row_src,
   xq, xd, xbsum, y).

   Numerics.  For a K-quant block j of row r: fp16 d and dmin widened to fp32; sc_g, mn_g the integer scale and min of group g
   (mn_g = 0 for Q3_K and Q6_K) and w_k the integer codes (signed for Q3_K and Q6_K) -- the quantities of ggml's
   dequantize_row_q*_K, value = d sc w - dmin mn:
     isum_j = sum_g sc_g * sum_{k in g} w_k * xq_k          exact in int32 (|isum| < 2^31: Q6_K at most 256 * 128 * 32 * 127)
     msum_j = sum_g mn_g * xbsum_g                          exact in int32
     term_j = xd[t, j] * (d * float(isum_j) - dmin * float(msum_j))      in fp32, each operation rounded once
   (Q3_K, Q6_K: term_j = xd[t, j] * (d * float(isum_j)).)  For GQ_Q8_0, with the eight 32-value blocks b of superblock j and
   their own d_b:  isum_b = sum_k w_k * xq_k exact;  term_j = xd[t, j] * (sum_b d_b * float(isum_b)), the sum over b in fp32
   in ascending b.
   The terms are added in fp32 in ascending j and the sum is rounded once (nearest even) to y_dtype.  The weight is never
   rounded to 16 bits.  Deterministic: one workgroup owns an output tile and walks all of C, no split across workgroups, no
   atomics.  The call only enqueues: no workspace, no allocation, no host synchronisation. */
int gq_linear_packed_a8(int q_type, const void* blocks, const int32_t* row_src, int64_t R, int64_t C,
                        const int8_t* xq, const float* xd, const int16_t* xbsum, int64_t T,
                        void* y, int y_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif
