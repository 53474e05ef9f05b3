/* gptq_gguf_kvcache.h -- a KV cache kept as Q8_0 blocks (8.5 bits per value) and the decode attention that reads it in that
   form: the append of new K / V rows and a split-KV attention for the few query tokens of a decode step.  An additive
   extension of the C ABI of gptq_gguf.h in the way of gptq_gguf_qgemv.h (same library, same conventions: status codes,
   gq_last_error, GQ_F16 / GQ_BF16, device pointers, `stream` a hipStream_t).  GQ_ABI_VERSION does not change. */
#ifndef GPTQ_GGUF_KVCACHE_H
#define GPTQ_GGUF_KVCACHE_H

#include "gptq_gguf_q8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_ATTN_DECODE_MAX_COLS 64 /* the most (query head of a group, query token) pairs G * T of one gq_attn_decode_q8_0 call */

/* ---- The cache layout.  Per layer, K and V are each one uint8 [B, Hkv, S_cap, D / 32 * 34] tensor: one cache row is one head
   vector of D values stored as D / 32 ggml Q8_0 blocks { fp16 d; int8 qs[32]; }, its bytes exactly what gq_quantize_q8_0
   writes for that row, so gq_dequantize_blocks(GQ_Q8_0, ...) on a (b, h) slab viewed as [S, D] is the reference decode.
   D is 64 or 128 (a row of 68 or 136 bytes); every other D is GQ_E_BAD_SHAPE.  The base pointers are 16-byte aligned and
   S_cap % 4 == 0, so every (b, h) slab starts 16-byte aligned and so does every run of positions that starts at a multiple
   of 4 (D = 64) or 2 (D = 128).  B, Hkv >= 1; B * Hkv * S_cap < 2^31 rows. */

/* ---- append: one launch encodes the T new K rows and the T new V rows into positions pos0 .. pos0 + T - 1 of both caches.
     k_new, v_new : [B, Hkv, T, D] in x_dtype GQ_F16 / GQ_BF16 with the strides new_sb, new_sh, new_st (in ELEMENTS, the same
                    for both tensors) of b, h and t; D has unit stride.  The transposed view [B, T, Hkv, D] -> [B, Hkv, T, D]
                    of an attention layer is passed as it is: nothing is copied.  Both pointers 16-byte aligned, every stride
                    a multiple of 8 elements (rows are read 16 bytes at a time).
     pos0         : a host integer, the length of the cache before the call; the host owns the length.
   The bytes written are bit for bit gq_quantize_q8_0's of each row (the contract of gptq_gguf_q8.h); no other byte of the
   caches is touched (2-byte stores that cover exactly the rows).  Refused before the first HIP call: GQ_E_BAD_TYPE x_dtype;
   GQ_E_NULL a null pointer; GQ_E_BAD_SHAPE D, B / Hkv / T < 1, S_cap % 4, pos0 < 0 or pos0 + T > S_cap, an alignment.
   The call only enqueues. */
int gq_kv_append_q8_0(const void* k_new, const void* v_new, int x_dtype, int64_t new_sb, int64_t new_sh, int64_t new_st,
                      int64_t B, int64_t Hkv, int64_t T, int64_t D, uint8_t* k_cache, uint8_t* v_cache, int64_t S_cap,
                      int64_t pos0, void* stream);

/* ---- decode attention: out[b, hq, t, :] = softmax(scale * q[b, hq, t] . K[b, hq / G, 0 .. pos0 + t]^T) V[b, hq / G, ...],
   G = Hq / Hkv.  The T query tokens sit at positions pos0 .. pos0 + T - 1, causal among themselves, over a cache of length
   pos0 + T: their own rows are already appended.
     q        : [B, Hq, T, D] in x_dtype with the element strides q_sb, q_sh, q_st (multiples of 8; 16-byte aligned); D unit.
     out      : contiguous [B, T, Hq, D] in x_dtype, 16-byte aligned -- the layout an attention function returns.
     kv_start : NULL or int32 [B] on the device: positions below kv_start[b] are masked (left padding).  The caller keeps
                kv_start[b] <= pos0, so that position pos0 + t is visible to token t: no column is fully masked.  No other
                mask form exists.
     ws       : gq_attn_decode_q8_0_workspace_bytes(pos0 + T, B, Hkv, G * T, D) bytes, 16-byte aligned.
   1 <= T, G * T <= GQ_ATTN_DECODE_MAX_COLS, Hq % Hkv == 0; everything else as for the append, refused in the same way
   (a short workspace is GQ_E_WORKSPACE).

   Numerics.  The K and V operand values are, bit for bit, gq_dequantize_blocks' for out_dtype = x_dtype: f32(d) * f32(q)
   rounded ONCE to the 16-bit type.  q . k products are exact in fp32 and accumulate in fp32 (matrix instructions); the scale
   is applied in fp32; the softmax (running maximum, exponentials, their sum) is fp32; the probabilities are rounded to x_dtype
   for the product with V, as every 16-bit flash kernel does, while their sum is taken before that rounding; the product
   accumulates in fp32, is normalised in fp32 and rounded once to x_dtype.  Masked positions contribute exactly zero.
   Deterministic: the split of the positions over workgroups is gq_attn_decode_q8_0_plan's, a function of (pos0 + T, B, Hkv,
   G * T) alone; partial results are merged in a fixed order, no atomics.  The same call gives the same bits.
   Two launches, no allocation, no host synchronisation. */
int gq_attn_decode_q8_0(const void* q, int x_dtype, int64_t q_sb, int64_t q_sh, int64_t q_st, int64_t B, int64_t Hq, int64_t Hkv,
                        int64_t T, int64_t D, const uint8_t* k_cache, const uint8_t* v_cache, int64_t S_cap, int64_t pos0,
                        const int32_t* kv_start, float scale, void* out, void* ws, size_t ws_bytes, void* stream);

/* 0 for arguments gq_attn_decode_q8_0 refuses.  S = pos0 + T, cols = G * T.  No HIP call. */
size_t gq_attn_decode_q8_0_workspace_bytes(int64_t S, int64_t B, int64_t Hkv, int64_t cols, int64_t D);

/* The plan of a call (csrc/attn/gq_attn_plan.hpp): positions [0, S) are cut into *splits chunks of *chunk positions (the last
   one shorter), one workgroup per (chunk, tile of 16 columns, KV head, batch row).  *min_chunk, *turn: a length up to
   *min_chunk is never split; a workgroup takes *turn positions per turn of its loop.  Any out pointer may be NULL. */
int gq_attn_decode_q8_0_plan(int64_t S, int64_t B, int64_t Hkv, int64_t cols, int64_t* splits, int64_t* chunk,
                             int64_t* min_chunk, int64_t* turn);

#ifdef __cplusplus
}
#endif
#endif
