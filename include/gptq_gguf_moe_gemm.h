/* gptq_gguf_moe_gemm.h -- the packed-weight forward of a mixture-of-experts layer's PREFILL: the router's (token, expert)
   pairs are sorted by expert on the device, and one tile GEMM launch over the stacked expert tensor serves every pair of a
   projection.  An additive extension of the C ABI of gptq_gguf.h in the way of gptq_gguf_moe.h (same library, same
   conventions: status codes, gq_last_error, GQ_F16 / GQ_BF16, device pointers, `stream` a hipStream_t).  GQ_ABI_VERSION does
   not change. */
#ifndef GPTQ_GGUF_MOE_GEMM_H
#define GPTQ_GGUF_MOE_GEMM_H

#include "gptq_gguf_moe.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_MOE_ROUTE_MAX_EXPERTS 256  /* the most experts gq_moe_route sorts by */
#define GQ_MOE_ROUTE_MAX_PAIRS 131072 /* the most (token, expert) pairs of one call: 16384 tokens at top-8 */

/* ---- a stable counting sort of the pairs by expert, entirely on the device.

   pair_expert: P int32 ON THE DEVICE, never read by the host: the router's [T, K] index in row-major order, the argument of
   gq_gemv_packed_experts.  An id outside [0, E) -- negative ids included; transformers uses E for a masked pair -- is valid
   input: such a pair appears nowhere in `order`.
   expert_start: E + 1 int32.  expert_start[e] is where expert e's run begins in `order`; expert_start[0] = 0 and
   expert_start[E] is the number of valid pairs.
   order: P int32.  Positions [expert_start[e], expert_start[e + 1]) hold the indices p of the pairs with pair_expert[p] == e,
   ASCENDING; every position from expert_start[E] on holds -1.
   Both outputs are fully defined for every input (compare them with an equality on the bits).

   1 <= E <= GQ_MOE_ROUTE_MAX_EXPERTS, 1 <= P <= GQ_MOE_ROUTE_MAX_PAIRS; the three pointers non-NULL and 4-byte aligned.
   Status codes as gq_gemv_packed_experts'; the checks run in the order NULL pointers, E, P, alignments and gq_last_error
   names the offending value (E=, P=).  Every check is made before the first HIP call: a refused call has launched nothing.

   Deterministic: the counts are integers (the order they are added in does not show), and a pair's position is its expert's
   start plus the number of EARLIER pairs of the same expert, taken from an ordered scan -- chunk by chunk of 1024 pairs,
   wave by wave, lane by lane --, never from the arrival order of an atomic.
   ONE launch of one workgroup whatever the data; no workspace beyond the two outputs, no allocation, no host synchronisation.
   Nothing outside pair_expert[0 .. P), expert_start[0 .. E] and order[0 .. P) is read or written. */
int gq_moe_route(const int32_t* pair_expert, int64_t P, int64_t E, int32_t* expert_start, int32_t* order, void* stream);

/* ---- for every pair p in order[0 .. expert_start[E]):   y[p, r] = sum_c x[p / pairs_per_row, c] * w[e, r, c],
   r = 0 .. R - 1, e the expert whose run [expert_start[e], expert_start[e + 1]) holds p.

   blocks, E, R, C, the alignments, x (contiguous [x_rows, C], x_rows * pairs_per_row == P) and y (contiguous [P, R]) as for
   gq_gemv_packed_experts, with 1 <= E <= GQ_MOE_ROUTE_MAX_EXPERTS and 1 <= P <= GQ_MOE_ROUTE_MAX_PAIRS.
   expert_start (E + 1 int32) and order (P int32) are what gq_moe_route wrote for the same P and E, ON THE DEVICE, never read
   by the host.  (The kernel trusts expert_start to be non-decreasing within [0, P]; an entry of `order` outside [0, P) is
   skipped, as -1 is.)
   The x rows are gathered through `order` and the y rows are scattered to pair order inside the kernel: no [n_e, C] copy of
   an expert's tokens exists.  Rows of y for pairs that are not in `order` are NOT written.  The weight bytes of an expert
   with an empty run are not read.

   ONE launch.  The host does not know the counts, so the grid is an upper bound: with TT tokens per tile,
   ceil(P / TT) + min(E, P) token tiles (sum_e ceil(n_e / TT) <= floor((N + k (TT - 1)) / TT) <= ceil(N / TT) + k - 1 for
   N = sum n_e <= P valid pairs on k <= min(E, P) hit experts) times ceil(R / 128) row tiles.  Every workgroup finds its
   (expert, tile) from expert_start -- E + 1 reads, one prefix sum inside a wave, no table in memory -- and one without work
   returns before any staging.  TT is 256 when P >= 128 * E (a run is on average at least 128 pairs long), else 128; Q4_K and
   Q5_K always take 128.  The result does not depend on TT.

   Status codes as gq_gemv_packed_experts'; the checks run in its order: q_type, x_dtype, NULL pointers, E, R, P, x_rows *
   pairs_per_row, C, alignments; gq_last_error names the offending value (E=, R=, P=, x_rows=, C=).  Every check is made
   before the first HIP call: a refused call has launched nothing.

   Nothing outside the blocks' extent, [x, x + x_rows * C * 2), expert_start[0 .. E], order[0 .. P) and [y, y + P * R * 2) is
   read or written.

   Numerics: row p of y is, BIT FOR BIT, what gq_linear_packed writes for (q_type, blocks + e * expert bytes, row_src = NULL,
   R, C, x + (p / pairs_per_row) * C elements, T = 1, x_dtype): the two kernels run one text (csrc/qgemm/gq_qgemm_core.hpp),
   in which an output element accumulates its own k sequence -- superblock, chunk, step, 32 k per matrix instruction --
   whatever the tile width, the token's place in the tile and the other tokens are.  So the result of a pair does not
   depend on which other pairs the call holds, on P or on the routing.  Deterministic: no atomics, no split-K across
   workgroups.  The call only enqueues: no workspace, no allocation, no host synchronisation. */
int gq_linear_packed_experts(int q_type, const void* blocks, int64_t E, int64_t R, int64_t C,
                             const void* x, int64_t x_rows, int64_t pairs_per_row,
                             const int32_t* expert_start, const int32_t* order, int64_t P,
                             int x_dtype, void* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif
