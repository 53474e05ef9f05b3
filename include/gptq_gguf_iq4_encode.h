/* gptq_gguf_iq4_encode.h -- the IQ4_NL / IQ4_XS encoder on the GPU: an additive extension of the C ABI of gptq_gguf.h in the way of
   gptq_gguf_q8.h (same library, same conventions: status codes, gq_last_error, GQ_F32 / GQ_F16 / GQ_BF16, device pointers,
   `stream` a hipStream_t).  GQ_ABI_VERSION does not change.  The layouts and the decode side are gptq_gguf_iq4.h's. */
#ifndef GPTQ_GGUF_IQ4_ENCODE_H
#define GPTQ_GGUF_IQ4_ENCODE_H

#include "gptq_gguf_iq4.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- encode: blocks[r, :] = encode(x[row_src ? row_src[r] : r, :]), r = 0 .. R - 1.
     x          contiguous [R, C] in x_dtype GQ_F32 / GQ_F16 / GQ_BF16, 16-byte aligned; widened exactly to fp32.
     q_type     GQ_IQ4_NL (C % 32 == 0) or GQ_IQ4_XS (C % 256 == 0); 32 <= C < 2^31, R >= 1.
     importance NULL, or C fp32 values on the device, 16-byte aligned, finite and >= 0, one per COLUMN: the value for output row r,
                column c is importance[c] (llama.cpp's importance matrix; the diagonal of the calibration Hessian is one).
     row_src    NULL (identity) or R int32 row indices on the device, each in [0, R) -- trusted, the kernel does not check.
     blocks     R * C / 32 blocks of 18 bytes (IQ4_NL) or R * C / 256 blocks of 136 bytes (IQ4_XS) in the layouts of
                gptq_gguf_iq4.h, 16-byte aligned (a workgroup stores 16 bytes at a time from the base on).  Nothing outside
                [blocks, blocks + R * row bytes) is written.
   GQ_E_BAD_TYPE for x_dtype and q_type, GQ_E_BAD_SHAPE for the shape rules and alignments above, GQ_E_NULL for x / blocks; every
   check is made before the first HIP call.  The call only enqueues: no allocation, no host synchronisation, no atomics.
   Non-finite inputs, and a d that overflows fp16, are outside the contract: the bytes written for such a block are unspecified.

   Contract (exact class).  ggml is not part of this project, so the algorithm below is THIS HEADER'S OWN CONTRACT, not a
   bit-for-bit claim about llama.cpp: it follows the ntry = 7 path of ggml's quantize_row_iq4_nl_impl, and comparing its bytes
   against a llama.cpp build is left to whoever has one.  The host form is gguf_writer.quantize_iq4 (numpy), byte for byte.

   All arithmetic is fp32, each operation rounded on its own (no contraction); divisions and sqrtf are correctly rounded; sums
   run in ascending j from 0.0f.  kv is the 16-entry table of gptq_gguf_iq4.h.

   best(a): 0 if a <= kv[0], 15 if a >= kv[15]; otherwise with u the smallest index with kv[u] > a: u - 1 if
     (a - kv[u-1]) < (kv[u] - a), both differences rounded to fp32, else u.  A tie goes up.  (The two rounded differences are
     compared, not a against a midpoint: a midpoint test is not bit-equal.)

   A super-block is 256 values for IQ4_XS and 32 for IQ4_NL, a block 32 values.
     sigma2 = (sum over the super-block of x[j]*x[j]) * (2.0f / size)
     weights of a block: without importance w[j] = x[j]*x[j]; with importance w[j] = importance[c_j] * sqrtf(sigma2 + x[j]*x[j]),
     unless every importance[c_j] of the block is 0: such a block takes the weights without importance.

   The scale d of a block:
     amax = max |x[j]|, max = the signed x[j] at the FIRST j that reaches it.  amax < 1e-15f: d = 0.  Otherwise, for an inverse
     scale id, with q[j] = kv[best(id * x[j])]:  sumqx = sum (w[j]*q[j])*x[j],  sumq2 = sum (w[j]*q[j])*q[j].
     First id = 1.0f / d0, d0 = -max / kv[0]:  d = sumqx / sumq2, best = d * sumqx.
     Then itry = -7 .. 7 in this order, id = (itry + kv[0]) / max: if sumq2 > 0 and sumqx*sumqx > best*sumq2 then
     d = sumqx / sumq2 and best = d * sumqx.

   IQ4_NL: the block stores fp16(d) (round-to-nearest-even); id = d != 0 ? 1.0f / d : 0 from the fp32 d; code j = best(id * x[j]);
     value j in the low nibble of qs[j], value j + 16 in the high nibble, j = 0 .. 15.
   IQ4_XS: ms = the block scale of largest |d| of the super-block, the first one on a tie (0 when all are 0); D = -ms / 32.0f,
     stored as fp16(D); iD = D != 0 ? 1.0f / D : 0.  Per block ib: l = clamp(rintf(iD * d_ib), -32, 31), dl = D * l from the fp32
     D, idl = dl != 0 ? 1.0f / dl : 0, codes best(idl * x[j]) as for IQ4_NL into qs[16 ib ..]; ls = l + 32 goes into scales_l /
     scales_h.
   Degenerate blocks: an all-zero block, and a block with l == 0, get code 8 everywhere (best(0) == 8); an all-zero super-block
   gets d == 0 (stored as -0 for IQ4_XS: D = -(+0) / 32).
   Results depend on the super-block's values and its importance only, never on the launch. */
int gq_quantize_iq4(const void* x, int x_dtype, int64_t R, int64_t C, int q_type, const float* importance, const int32_t* row_src,
                    uint8_t* blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif
