/* gptq_gguf_iq4.h -- IQ4_NL and IQ4_XS, ggml's two 4-bit non-linear types, read on the GPU: an additive extension of the C ABI
   of gptq_gguf.h in the way of gptq_gguf_q8.h (same library, same conventions: status codes, gq_last_error, GQ_F32 / GQ_F16 /
   GQ_BF16, device pointers, `stream` a hipStream_t).  There is NO new symbol and GQ_ABI_VERSION does not change: the header
   carries two type ids, their layouts and the rules under which the existing decode and packed-forward entry points take
   them.  The encoder of both types is gq_quantize_iq4 of gptq_gguf_iq4_encode.h; levels of these types also come from files that
   llama.cpp quantized. */
#ifndef GPTQ_GGUF_IQ4_H
#define GPTQ_GGUF_IQ4_H

#include "gptq_gguf_q8.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The ggml type ids; free among GQ_F32 / GQ_F16 / GQ_BF16 (0 / 1 / 2), GQ_Q8_0 (8) and GQ_Q2_K .. GQ_Q6_K (10 .. 14). */
#define GQ_IQ4_NL 20
#define GQ_IQ4_XS 23

/* Both types map a 4-bit code through one table (ggml's kvalues_iq4nl):
     kv[16] = { -127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113 }

   IQ4_NL (dequantize_row_iq4_nl): a block is 32 values in 18 bytes, natural alignment 2; C % 32 == 0.
     { fp16 d; uint8 qs[16]; }
     j = 0 .. 15:  y[j] = d * kv[qs[j] & 15],  y[j + 16] = d * kv[qs[j] >> 4]

   IQ4_XS (dequantize_row_iq4_xs): a superblock is 256 values in 136 bytes; C % 256 == 0.  A block's address is 8-byte
   aligned in a GGUF file (32-byte tensor alignment, 136 = 17 * 8) and in a level file.
     { fp16 d; uint16 scales_h; uint8 scales_l[4]; uint8 qs[128]; }
     sub-block ib = 0 .. 7 of 32 values:
       ls = ((scales_l[ib / 2] >> 4 * (ib % 2)) & 15) | (((scales_h >> 2 * ib) & 3) << 4),  dl = d * (ls - 32)
       j = 0 .. 15, q = qs[16 ib + j]:  y[32 ib + j] = dl * kv[q & 15],  y[32 ib + 16 + j] = dl * kv[q >> 4]

   Contract (exact class): computed in fp32, then ONE round-to-nearest-even cast to the output dtype.  Both products are exact
   in fp32 -- 11 significant bits of d times at most 6 of (ls - 32) times at most 7 of kv is at most 24 --, so the order of the
   multiplications does not show, and neither overflow nor underflow can occur in fp32: the result is bit for bit torch's
   `(d.float() * (ls - 32).float() * kv.float()).to(dtype)`.  A non-finite d propagates as it does there: inf * 0 is NaN when
   ls == 32; kv is never 0.  Every bit pattern of the other fields is a valid block.

   ---- decode: gq_dequantize_blocks (gptq_gguf.h) and gq_level_switch (gptq_gguf_search.h) take q_type / kind GQ_IQ4_NL and
   GQ_IQ4_XS, with the row_src gather and all three output dtypes.
     blocks / src : IQ4_NL: R rows of C / 32 blocks of 18 bytes, C % 32 == 0, 2-byte aligned; staging loads are 2 bytes wide.
                    IQ4_XS: R rows of C / 256 blocks of 136 bytes, C % 256 == 0, 8-byte aligned; staging loads are 8 bytes wide.
                    The loads cover exactly the blocks' bytes: nothing outside [src, src + R * row bytes) is read.
     out / dst    : contiguous [R, C], 16-byte aligned.
   GQ_E_BAD_SHAPE for these rules, as for GQ_Q8_0; every check is made before the first HIP call.  The unit of
   gq_level_switch's accounting for a job of either type is 4096 values (128 blocks of IQ4_NL, 16 of IQ4_XS).

   ---- packed forward: gq_linear_packed (gptq_gguf_qgemm.h), gq_gemv_packed (gptq_gguf_qgemv.h), gq_gemv_packed_experts
   (gptq_gguf_moe.h) and gq_linear_packed_experts (gptq_gguf_moe_gemm.h) take both types.  C % 256 == 0 is required there for
   IQ4_NL too, as for Q8_0; the alignment of `blocks` is the type's (2 / 8 bytes).  The weight operand is bit for bit what
   gq_dequantize_blocks writes; everything else in those headers' contracts holds unchanged (fp32 accumulation, one rounding,
   deterministic, the grouped kernels bit-equal to their single-matrix kernels).

   Every other entry point that takes a q_type -- gq_pack, gq_unpack, gq_rtn_quantize, gq_type_info, the walks, gq_pack_bands,
   gq_quantize_q8_0 -- keeps refusing 20 and 23 with GQ_E_BAD_TYPE.  The other IQ types (IQ1, IQ2, IQ3) need ggml's grid
   tables and are not read. */

#ifdef __cplusplus
}
#endif
#endif
