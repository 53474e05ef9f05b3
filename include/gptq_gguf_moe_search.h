/* gptq_gguf_moe_search.h -- the level switch of the bit-width search for the stacked expert tensors of a mixture-of-experts
   model: one job makes a whole `blk.N.ffn_{gate,up,down}_exps.weight` current.  An additive extension of the C ABI of
   gptq_gguf.h in the way of gptq_gguf_moe_calib.h (same library, same conventions: status codes, gq_last_error, GQ_F32 /
   GQ_F16 / GQ_BF16, device pointers, `stream` a hipStream_t).  GQ_ABI_VERSION does not change. */
#ifndef GPTQ_GGUF_MOE_SEARCH_H
#define GPTQ_GGUF_MOE_SEARCH_H

#include "gptq_gguf_iq4.h" /* (includes gptq_gguf_q8.h and gptq_gguf_search.h) */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- one stored level of a stacked expert tensor decoded or cast into the E live matrices of its role.

   A job:   for e = 0 .. E - 1:   D_e[r, :] = convert(S_e[r, :]),   r = 0 .. R - 1, where
     S_e is expert e's slice of `src`, the tensor as it lies in a GGUF file or a level file: E * R rows of packed blocks
         (slice e starts at src + e * R * row bytes), or a dense contiguous [E, R, C] tensor;
     D_e is the contiguous [R, C] matrix of `out_dtype` at dst + e * dst_expert_stride ELEMENTS of out_dtype.
   dst_expert_stride >= R * C and dst_expert_stride * element size % 16 == 0.  The stride is what lets one job fill the gate
   half or the up half of transformers' fused gate_up_proj [E, 2I, H] (gate: rows [0, I) of every expert, dst = the
   parameter; up: rows [I, 2I), dst = the parameter + I * H elements; both with stride 2 * I * H) as well as down_proj
   [E, H, I] (stride H * I).  There is no row_src: expert tensors carry no rotary permutation.

   kind: every kind gq_level_switch takes -- GQ_Q2_K .. GQ_Q6_K, GQ_Q8_0, GQ_IQ4_NL, GQ_IQ4_XS, or a dense source
   GQ_F32 / GQ_F16 / GQ_BF16.

   Contract: the values are, bit for bit, those of gq_level_switch called with the E jobs
       (src + e * slice bytes, dst + e * dst_expert_stride, NULL, R, C, kind, out_dtype),
   whose turn this kernel runs (the same text).  Nothing is written outside the E matrices D_e -- the other half of
   gate_up_proj in particular is untouched --, nothing is read outside [src, src + E * R * row bytes).
   The rules per kind are gq_level_switch's, applied to every expert's slice: C % 256 == 0 (GQ_Q8_0 / GQ_IQ4_NL: C % 32 == 0;
   dense: both row sizes multiples of 16 bytes); src aligned to the type (Q2_K 4 bytes, Q3_K / Q6_K / Q8_0 / IQ4_NL 2,
   IQ4_XS 8, Q4_K / Q5_K and dense 16) and R * row bytes a multiple of that alignment when E > 1 (every block type's size
   is a multiple of its alignment, so this refuses nothing gq_level_switch takes); dst 16 bytes.
   1 <= E <= 65535, R >= 1, 1 <= C < 2^31; E times the work units of one expert (a unit: 4096 values of a packed kind, 512
   16-byte stores of a dense one; units never straddle experts) must fit one launch (2^31 - 1).
   Anything else is GQ_E_BAD_SHAPE (GQ_E_NULL / GQ_E_BAD_TYPE for pointers / kind / out_dtype); gq_last_error names the
   job index and the argument.  Every check is made before the first HIP call, for all jobs: a refused call has launched
   nothing.

   The table `jobs_host` is a HOST array, read during the call: it travels in the kernel arguments, no staging buffer and
   no copy is put on the stream.  n_jobs >= 0; the list is cut into launches of at most GQ_SWITCH_EXPERTS_MAX_JOBS jobs (the
   largest count whose table fits the 4 KB kernel-argument segment); n_jobs == 0 is a successful no-op without a launch.
   Jobs of one call must not overlap in dst.  A workgroup maps its unit to (job, expert, unit in the expert) with
   block-uniform arithmetic.  The call only enqueues: no workspace, no host synchronisation, no allocation, no atomics. */
#define GQ_SWITCH_EXPERTS_MAX_JOBS 71

typedef struct {
    const void* src;
    void* dst;
    int64_t E, R, C;
    int64_t dst_expert_stride; /* elements of out_dtype between expert e's and expert e + 1's destination matrix */
    int32_t kind;              /* GQ_Q2_K..GQ_Q6_K, GQ_Q8_0, GQ_IQ4_NL, GQ_IQ4_XS packed blocks, or GQ_F32 / GQ_F16 / GQ_BF16 dense */
    int32_t out_dtype;         /* GQ_F32 / GQ_F16 / GQ_BF16 */
} gq_switch_experts_job_t;

int gq_level_switch_experts(const gq_switch_experts_job_t* jobs_host, int n_jobs, void* stream);

#ifdef __cplusplus
}
#endif
#endif
