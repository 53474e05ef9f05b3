/* gptq_gguf_kvprefill.h -- the attention of MANY query tokens over the Q8_0 KV cache of gptq_gguf_kvcache.h: a chunk of a long
   prompt, or a later turn of a conversation, read at the cache's stored size.  gq_attn_decode_q8_0 takes at most
   GQ_ATTN_DECODE_MAX_COLS columns; this call takes any number.  An additive extension of the C ABI in the way of
   gptq_gguf_kvcache.h (same library, same conventions); GQ_ABI_VERSION does not change. */
#ifndef GPTQ_GGUF_KVPREFILL_H
#define GPTQ_GGUF_KVPREFILL_H

#include "gptq_gguf_kvcache.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- prefill attention: out[b, hq, t, :] = softmax(scale * q[b, hq, t] . K[b, hq / G, 0 .. pos0 + t]^T) V[b, hq / G, ...],
   G = Hq / Hkv, for the T query tokens at positions pos0 .. pos0 + T - 1, causal among themselves, over a cache of length
   pos0 + T: their own rows are already appended.  Operands, layout, checks and status codes are gq_attn_decode_q8_0's:
     q        : [B, Hq, T, D] in x_dtype with the element strides q_sb, q_sh, q_st (multiples of 8; 16-byte aligned); D unit.
     k_cache, v_cache : uint8 [B, Hkv, S_cap, D / 32 * 34], the layout of gptq_gguf_kvcache.h; D is 64 or 128.
     out      : contiguous [B, T, Hq, D] in x_dtype, 16-byte aligned.
     kv_start : NULL or int32 [B] on the device: positions below kv_start[b] are masked (left padding).  Unlike the decode
                call, kv_start[b] may exceed pos0, up to pos0 + T -- a left-padded first chunk: a query token whose position
                lies below kv_start[b] sees nothing and its output row is exactly zero.
   Any T >= 1, any G >= 1, any pos0 >= 0 (G * T and the number of workgroups below 2^31).  There is no workspace.

   Numerics: the contract of gq_attn_decode_q8_0.  The K and V operand values are, bit for bit, gq_dequantize_blocks' for
   out_dtype = x_dtype (one rounding); q . k accumulates in fp32 on matrix instructions; the scale and the online softmax are
   fp32; the probabilities are rounded to x_dtype for the product with V while their sum is taken before that rounding; the
   product accumulates in fp32, is normalised in fp32 and rounded once.  Masked positions and rows past pos0 + T contribute
   exactly zero, whatever their bytes.  Every column is computed by one workgroup that walks the positions in rising order:
   nothing is merged, there are no atomics, and the same call gives the same bits.
   One launch, no allocation, no host synchronisation; every refusal is made before the first HIP call. */
int gq_attn_prefill_q8_0(const void* q, int x_dtype, int64_t q_sb, int64_t q_sh, int64_t q_st, int64_t B, int64_t Hq, int64_t Hkv,
                         int64_t T, int64_t D, const uint8_t* k_cache, const uint8_t* v_cache, int64_t S_cap, int64_t pos0,
                         const int32_t* kv_start, float scale, void* out, void* stream);

/* The plan of a call (csrc/attn/gq_attn_prefill_plan.hpp): the G * T columns c = t * G + g of a KV head are cut into *blocks
   blocks of *block_cols columns, one workgroup per (block, batch row, KV head), launched last block first; a workgroup takes
   *turn positions per turn of its walk.  Any out pointer may be NULL.  No HIP call. */
int gq_attn_prefill_q8_0_plan(int64_t T, int64_t G, int64_t* block_cols, int64_t* turn, int64_t* blocks);

#ifdef __cplusplus
}
#endif
#endif
