/* gptq_gguf_qgemv_group_a8.h -- the projections of ONE input in one launch, on int8 activations: up to four packed weights
   (q / k / v of an attention block; gate / up of a dense MLP) share x, which every workgroup quantizes once, and the
   gate / up form applies SwiGLU in the epilogue.  gq_gemv_packed_a8's arithmetic (gptq_gguf_qgemv_a8.h) on a grid that is
   partitioned among the members.  An additive extension of the C ABI of gptq_gguf.h (same library, same conventions: status
   codes, gq_last_error, GQ_F16 / GQ_BF16, device pointers, `stream` a hipStream_t).  GQ_ABI_VERSION does not change.  Every
   check is made before the first HIP call: a refused call has launched nothing. */
#ifndef GPTQ_GGUF_QGEMV_GROUP_A8_H
#define GPTQ_GGUF_QGEMV_GROUP_A8_H

#include "gptq_gguf_qgemv_a8.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_GEMV_GROUP_MAX 4    /* the most members of one call */
#define GQ_GEMV_GROUP_SPLIT 0  /* every member writes its own y[T, R_m] */
#define GQ_GEMV_GROUP_SWIGLU 1 /* exactly two members (gate, up): member 0's y receives act[T, R] */

/* One member: gq_gemv_packed_a8's (q_type, blocks, row_src, R, y) of one weight [R, C].  `members` is a HOST array: the call
   copies it into the kernel's arguments (as gq_level_switch does with its job table), so it may be freed or reused as soon as
   the call returns.  blocks, row_src (may be NULL) and y are device pointers. */
typedef struct {
    int q_type;
    const void* blocks;
    const int32_t* row_src;
    int64_t R;
    void* y;
} gq_gemv_member_t;

/* ---- one launch for the n_members weights of x [T, C] (contiguous, x_dtype), 1 <= T <= GQ_GEMV_A8_MAX_T, C % 256 == 0.
   q_type of a member: GQ_Q2_K .. GQ_Q6_K or GQ_Q8_0, in any mixture; GQ_IQ4_NL and GQ_IQ4_XS are NOT served: GQ_E_BAD_TYPE, the
   message names the type and the member.

   GQ_GEMV_GROUP_SPLIT.  Member m's y is contiguous [T, R_m] in x_dtype, and row r of it is BIT FOR BIT what
   gq_gemv_packed_a8(q_type_m, blocks_m, row_src_m, R_m, C, x, T, x_dtype, y_m, ..) writes: the same quantized image of x, the
   same terms, the same fp32 order, one rounding (gptq_gguf_qgemv_a8.h states every operation).
   GQ_GEMV_GROUP_SWIGLU.  n_members == 2 (gate, up) with equal R and equal q_type, members[1].y == NULL.  members[0].y receives
   act [T, R], BIT FOR BIT gq_fwd_silu_mul(G, U) where G and U are the two gq_gemv_packed_a8 outputs: each sum is rounded once
   to x_dtype, then act = round(round(silu(G)) * U) with silu(g) = g / (1 + expf(-g)) in fp32 (the two roundings of
   gq_fwd_silu_mul and of gq_silu_mul_quantize_act_q8).  G and U are never written.

   Checks, in this order, each naming its argument (a member's as members[m].<field>):
     mode; n_members (1 .. GQ_GEMV_GROUP_MAX); members NULL; x_dtype; per member m in order: q_type (IQ4 by name, then unknown);
     SWIGLU's shape: n_members == 2, members[1].q_type == members[0].q_type, members[1].y == NULL;
     NULL: per member blocks, then y (SWIGLU: members[0].y only); x;
     per member R; SWIGLU: members[1].R == members[0].R; T; C; the image (T * C * 73 / 64 bytes of LDS, as gq_gemv_packed_a8);
     alignments: per member blocks (the type's: 16 for Q4_K / Q5_K, 4 for Q2_K, 2 otherwise), row_src (4), y (16); x (16).
   Nothing outside the members' blocks, [x, x + T * C * 2) and each written [y, y + T * R * 2) is read or written.

   Deterministic: a wave owns whole rows, no atomics, plain vector stores; a row's result depends on its row and on x only, not
   on the other members or on the partition of the grid (gq_gemv_group_a8_plan).  The call only enqueues: one launch, no
   device table, no workspace, no allocation, no host synchronisation. */
int gq_gemv_packed_group_a8(const gq_gemv_member_t* members, int n_members, int64_t C, const void* x, int64_t T, int x_dtype,
                            int mode, void* stream);

/* ---- how gq_gemv_packed_group_a8 would run, without a device: lds_bytes of the image, grid (workgroups of 16 waves, at most
   256), first_wg [n_members + 1] and fits (1 / 0: the image is within the LDS budget).  Any output pointer may be NULL.
   SPLIT: member m owns workgroups [first_wg[m], first_wg[m + 1]), first_wg[n_members] = grid, and workgroup b of its g_m walks
   its row groups of 16 rows b, b + g_m, ..  The partition is by largest remainder on the weight bytes:
     cap_m = ceil(R_m / 16);  grid = min(256, sum cap_m);  quota_m = grid * bytes_m / sum bytes,  bytes_m = R_m * (row bytes of q_type_m at C)
     g_m = min(max(floor(quota_m), 1), cap_m);  while sum g_m < grid: one more to the member with g_m < cap_m and the largest
     quota_m - g_m (a tie: the lowest m);  while sum g_m > grid: one less for the member with g_m > 1 and the smallest
     quota_m - g_m (a tie: the highest m).  Exact integer comparisons.
   SWIGLU: the two members share every workgroup (a wave walks gate row r and up row r back to back):
     grid = min(256, cap_0) and first_wg = {0, 0, grid}.
   The checks of gq_gemv_packed_group_a8 on mode, n_members, q_types, R, T and C apply (SWIGLU's shape included). */
int gq_gemv_group_a8_plan(const int* q_types, const int64_t* R, int n_members, int64_t C, int64_t T, int mode,
                          int64_t* lds_bytes, int64_t* grid, int64_t* first_wg, int64_t* fits);

#ifdef __cplusplus
}
#endif
#endif
