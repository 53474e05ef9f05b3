/* gptq_gguf_moe.h -- the packed-weight forward of a mixture-of-experts layer's decode step: one GEMV launch over the stacked
   expert tensor for every (token, expert) pair of the step.  An additive extension of the C ABI of gptq_gguf.h in the way of
   gptq_gguf_qgemv.h (same library, same conventions: status codes, gq_last_error, GQ_F16 / GQ_BF16, device pointers, `stream`
   a hipStream_t).  GQ_ABI_VERSION does not change. */
#ifndef GPTQ_GGUF_MOE_H
#define GPTQ_GGUF_MOE_H

#include "gptq_gguf_qgemv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_MOE_MAX_PAIRS 64 /* the most (token, expert) pairs of one gq_gemv_packed_experts call */

/* ---- y[p, r] = sum_c x[p / pairs_per_row, c] * w[pair_expert[p], r, c],   p = 0 .. P - 1,   r = 0 .. R - 1.

   blocks: E experts of R rows of C / 256 blocks (Q8_0: C / 32 of 34 bytes), contiguous and expert-major: a GGUF [E, R, C]
   tensor (`blk.N.ffn_{gate,up,down}_exps.weight`) as it lies in the file, at the block's natural alignment (Q2_K 4 bytes,
   Q3_K / Q6_K / Q8_0 2, Q4_K / Q5_K 16).  An expert's byte stride R * (C / 256) * (84, 110, 144, 176, 210 or 272) is a
   multiple of that alignment for all six types (84 = 4 * 21, 144 = 16 * 9, 176 = 16 * 11, the others even), so every
   expert's slice is aligned when the tensor is.  q_type GQ_Q2_K .. GQ_Q6_K or GQ_Q8_0; 1 <= E <= 65535; R, C, x_dtype and the
   alignments of x and y as for gq_gemv_packed (1 <= R < 2^31; C % 256 == 0, 256 <= C < 2^31; GQ_F16 or GQ_BF16; 16 bytes).
   There is no row_src: the rows of an expert FFN are never permuted.

   pair_expert: P int32 ON THE DEVICE, never read by the host.  Pair p multiplies expert pair_expert[p] with row
   p / pairs_per_row of x (contiguous [x_rows, C]) and writes row p of y (contiguous [P, R]); x_rows * pairs_per_row == P is
   required, 1 <= P <= GQ_MOE_MAX_PAIRS.  pairs_per_row = K serves the gate and up projections of a top-K layer (x the hidden
   states [T, H], the pairs in the row-major order of the router's [T, K] index); pairs_per_row = 1 serves the down
   projection (x the [P, I] activation).
   A pair_expert value outside [0, E) is NOT checked and is no error: that pair is skipped, its row of y is not written
   (transformers uses the id E for a masked pair).  The weight bytes of an expert that no pair names are not read.

   Status codes as gq_gemv_packed's; the checks run in the order q_type, x_dtype, NULL pointers, E, R, P, x_rows *
   pairs_per_row, C, alignments; gq_last_error names the offending value (E=, R=, P=, x_rows=, C=).  Every check is made
   before the first HIP call: a refused call has launched nothing.

   Nothing outside the blocks' extent, [x, x + x_rows * C * 2), pair_expert[0 .. P) and [y, y + P * R * 2) is read or written.

   Numerics: row p of y is, BIT FOR BIT, what gq_gemv_packed writes for (q_type, blocks + pair_expert[p] * expert bytes,
   row_src = NULL, R, C, x + (p / pairs_per_row) * C elements, T = 1, x_dtype): the two kernels run one text (K split over
   the waves of the workgroup that owns 16 rows, fixed wave-order reduction, one rounding), and a column of the matrix
   instruction depends on its own input row only.  So the result of a pair does not depend on which other pairs the call
   holds, on P or on the order of the pairs.  Deterministic: no atomics, no split across workgroups.
   The call only enqueues: no workspace, no allocation, no host synchronisation. */
int gq_gemv_packed_experts(int q_type, const void* blocks, int64_t E, int64_t R, int64_t C,
                           const void* x, int64_t x_rows, const int32_t* pair_expert, int64_t P,
                           int64_t pairs_per_row, int x_dtype, void* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif
