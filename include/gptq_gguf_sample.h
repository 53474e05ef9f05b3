/* gptq_gguf_sample.h -- one launch from a logits matrix to token ids: temperature, top-k, top-p and the draw, with the random
   number supplied by the caller.  An additive extension of the C ABI of gptq_gguf.h in the way of gptq_gguf_qgemv.h (same
   library, same conventions: status codes, gq_last_error, GQ_F32 / GQ_F16 / GQ_BF16, device pointers, `stream` a
   hipStream_t).  GQ_ABI_VERSION does not change. */
#ifndef GPTQ_GGUF_SAMPLE_H
#define GPTQ_GGUF_SAMPLE_H

#include "gptq_gguf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_SAMPLE_MAX_K 1024 /* the largest top_k: the candidates of a row live in one workgroup's LDS */

/* ---- ids[b] = the token drawn from row b of logits, b = 0 .. B - 1.
   logits follows the gq_eval_* calls: row b starts at logits + b * ld elements, ld >= V, dtype GQ_F32, GQ_F16 or GQ_BF16, only
   element alignment is required and nothing outside [row, row + V) is read.  u: B floats on the device, each in [0, 1), the
   caller's random numbers (4-byte aligned); may be NULL when temperature == 0.  ids: B int64 on the device (8-byte aligned).

   Per row, where everything but two fp32 sums is exact:
     1. z_i = f32(logit_i) (exact).  Tokens are ranked by (z descending, index ascending); -0 and +0 are equal.
     2. A NaN in the row, or a maximum that is not finite (+inf, or a row of -inf): ids[b] = -1, nothing else is done.
     3. The candidates are the first K = min(top_k, V) tokens of that order.
     4. temperature == 0: the rank-0 token -- the argmax, the lowest index among equal maxima.
     5. Otherwise, in fp32 and in rank order: w_j = exp((z_j - z_0) / temperature), S = sum_{j < K} w_j.  The nucleus is the
        smallest n with sum_{j < n} w_j >= top_p * S (top_p == 1: n = K).  The result is the smallest j < n with
        sum_{i <= j} w_i > u * sum_{i < n} w_i; if rounding leaves no such j, the largest j < n with w_j > 0.
        This is the order of HF's logits processors: temperature, then top-k, then top-p.  A -inf candidate has w = 0 and is
        never returned.
   Neither the summation order of the prefix sums nor the exp used is promised: a token is pinned exactly whenever u * S_n and
   top_p * S are not within fp32 rounding of a prefix sum.  The ranking, the candidate set (ties at the K-th place go to the
   lowest indices) and the argmax are exact always.

   An unbounded nucleus (top_k = 0, "no top-k") is deliberately not built: top_k must be in [1, GQ_SAMPLE_MAX_K].

   Refusals, all made before the first HIP call (a refused call has launched nothing): dtype not one of the three
   GQ_E_BAD_TYPE; logits or ids NULL, or u NULL with temperature > 0, GQ_E_NULL; GQ_E_BAD_SHAPE for B < 1, V < 1, B or V >= 2^31,
   ld < V, top_k outside [1, GQ_SAMPLE_MAX_K], top_p outside (0, 1] or NaN, temperature < 0 or NaN, and a misaligned pointer.
   gq_last_error names the call and the value.

   Deterministic: one workgroup owns a row; counts are integer adds in LDS, the sums are added in a fixed order.  The same
   call gives the same bits.  The call only enqueues: no workspace, no allocation, no host synchronisation, no atomics on
   global memory. */
int gq_sample_logits(const void* logits, int dtype, int64_t B, int64_t V, int64_t ld, int top_k, float top_p, float temperature,
                     const float* u, int64_t* ids, void* stream);

#ifdef __cplusplus
}
#endif
#endif
