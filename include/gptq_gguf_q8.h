/* gptq_gguf_q8.h -- Q8_0 (block_q8_0 { fp16 d; int8 qs[32]; }, 34 bytes per 32 values, 8.5 bits per weight) on the GPU:
   an additive extension of the C ABI of gptq_gguf.h (same library, same conventions: status codes, gq_last_error,
   GQ_F32 / GQ_F16 / GQ_BF16, device pointers, `stream` a hipStream_t).  GQ_ABI_VERSION does not change.  The symbols live
   in a header of their own so that gptq_gguf.h stays the symbol set its version names. */
#ifndef GPTQ_GGUF_Q8_H
#define GPTQ_GGUF_Q8_H

#include "gptq_gguf_search.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The ggml type id, as GQ_Q2_K .. GQ_Q6_K (10 .. 14) are; free among them and GQ_F32 / GQ_F16 / GQ_BF16 (0 / 1 / 2). */
#define GQ_Q8_0 8

/* ---- decode: gq_dequantize_blocks (gptq_gguf.h) and gq_level_switch (gptq_gguf_search.h) take q_type / kind GQ_Q8_0.
     blocks / src : R rows of C / 32 blocks of 34 bytes; C % 32 == 0 (not 256); 2-byte aligned, the block's natural
                    alignment.  Staging loads are 2 bytes wide and cover exactly the blocks' bytes: nothing outside
                    [src, src + R * C / 32 * 34) is read.
     out / dst    : contiguous [R, C], 16-byte aligned.  row_src as for the K-quants: out[r] = decode(src row row_src[r]).
   Contract (exact class): w = f32(d) * f32(q) -- exact in fp32, 11 significant bits times 7 --, then ONE round-to-
   nearest-even cast to the output dtype: torch's `d.float() * q.float()` followed by `.to(dtype)`, bit for bit.  A
   non-finite d propagates as there (inf * 0 = NaN).  The unit of gq_level_switch's accounting for such a job is 128 blocks
   of 32 values, the 4096 values of a K-quant unit.
   Every other entry point that takes a q_type (gq_pack, gq_unpack, gq_rtn_quantize, gq_type_info, the walks,
   gq_pack_bands) keeps refusing 8 with GQ_E_BAD_TYPE. */

/* ---- encode: blocks[r, :] = encode(x[row_src ? row_src[r] : r, :]), r = 0 .. R - 1.
     x       contiguous [R, C] in x_dtype GQ_F32 / GQ_F16 / GQ_BF16, 16-byte aligned; widened exactly to fp32.
     blocks  R * C / 32 blocks of 34 bytes, 16-byte aligned (a workgroup stores 16 bytes at a time from the base on).
     row_src NULL (identity) or R int32 row indices on the device, each in [0, R) -- trusted, the kernel does not check.
     C % 32 == 0, 32 <= C < 2^31, R >= 1.
   Contract (exact class), per block of 32 values -- ggml-quants.c quantize_row_q8_0_ref, bit for bit:
     amax = max |x|;  d = amax / 127.0f, a correctly rounded fp32 division;  id = d != 0 ? 1.0f / d : 0;
     q = roundf(x * id), rounding half away from zero (the product with id, not a division by d);
     d is stored as fp16 by round-to-nearest-even: it may round to 0 or overflow to inf while the codes come from the fp32 d.
   Behaviour on non-finite inputs (NaN, inf) is outside the contract: the bytes written for such a block are unspecified.
   GQ_E_BAD_SHAPE for the shape rules and alignments above, GQ_E_BAD_TYPE for x_dtype, GQ_E_NULL for x / blocks; every check
   is made before the first HIP call.  The call only enqueues: no allocation, no host synchronisation, no atomics. */
int gq_quantize_q8_0(const void* x, int x_dtype, int64_t R, int64_t C, const int32_t* row_src, uint8_t* blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif
