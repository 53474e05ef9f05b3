/* gptq_gguf_search.h -- the level switch of the per-layer bit-width search (evopress/evo_quant_search.py): an additive
   extension of the C ABI of gptq_gguf.h (same library, same conventions: status codes, gq_last_error, GQ_F32 / GQ_F16 /
   GQ_BF16, device pointers, `stream` a hipStream_t).  GQ_ABI_VERSION does not change.  The symbol lives in a header of
   its own so that gptq_gguf.h stays the symbol set its version names. */
#ifndef GPTQ_GGUF_SEARCH_H
#define GPTQ_GGUF_SEARCH_H

#include "gptq_gguf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- one candidate of the search made current (replaces load_layers, evopress/evo_quant_search.py:110-138: a torch.load of a
   dense [R, C] file and a .to(dtype) per changed Linear): every job decodes or casts one stored level straight into the
   live weight.

   A job:   dst[r, :] = convert(src[row_src ? row_src[r] : r, :]),   r = 0 .. R - 1,   dst contiguous [R, C] in out_dtype.
     kind GQ_Q2_K .. GQ_Q6_K : src holds R rows of C / 256 packed blocks; the values are, bit for bit, those of
                               gq_dequantize_blocks for the same (q_type, blocks, R, C, row_src, out_dtype).  C % 256 == 0;
                               src aligned to the block's natural alignment (Q2_K 4 bytes, Q3_K / Q6_K 2, Q4_K / Q5_K 16),
                               dst 16 bytes.  Staging loads cover exactly the blocks' bytes: nothing outside
                               [src, src + R * C / 256 * type_size) is read, nothing outside [dst, dst + R * C * elsize)
                               is written.
     kind GQ_F32 / GQ_F16 / GQ_BF16 : src is a dense contiguous [R, C] matrix of that dtype; a cast copy, widened exactly to
                               fp32 and rounded once to nearest-even (torch's .to(dtype)).  src, dst and both row sizes
                               (C * element size) must be multiples of 16 bytes.
     kind GQ_Q8_0 (gptq_gguf_q8.h) : src holds R rows of C / 32 blocks of 34 bytes, 2-byte aligned, C % 32 == 0; the unit is 128
                               such blocks.  That header states the contract.
     kind GQ_IQ4_NL / GQ_IQ4_XS (gptq_gguf_iq4.h) : R rows of C / 32 blocks of 18 bytes, 2-byte aligned, C % 32 == 0 / of
                               C / 256 blocks of 136 bytes, 8-byte aligned, C % 256 == 0; the unit is 4096 values.  That
                               header states the contract.
   row_src: NULL (identity) or R int32 row indices on the device, each in [0, R) -- the kernel does not check.
   R >= 1.  Anything else is GQ_E_BAD_SHAPE (GQ_E_NULL / GQ_E_BAD_TYPE for pointers / kind / out_dtype); gq_last_error
   names the job index and the argument.  Every check is made before the first HIP call, for all jobs: a refused call has
   launched nothing.

   The table `jobs_host` is a HOST array, read during the call: it travels in the kernel arguments, no staging buffer and
   no copy is put on the stream.  n_jobs >= 0; the list is cut into launches of at most GQ_SWITCH_MAX_JOBS jobs (the
   table of that many jobs fits the 4 KB kernel-argument segment); n_jobs == 0 is a successful no-op without a launch.
   Jobs of one call must not overlap in dst.  A workgroup finds its job by a search over the prefix sum of work units in
   the table (unit: 16 blocks of 256 values, the turn of the K15 decode kernel; dense jobs: 512 16-byte stores).  The call only
   enqueues: no host synchronisation, no allocation, no atomics. */
#define GQ_SWITCH_MAX_JOBS 64

typedef struct {
    const void* src;
    void* dst;
    const int32_t* row_src; /* NULL = identity */
    int64_t R, C;
    int32_t kind;      /* GQ_Q2_K..GQ_Q6_K packed blocks, or GQ_F32 / GQ_F16 / GQ_BF16 dense source */
    int32_t out_dtype; /* GQ_F32 / GQ_F16 / GQ_BF16 */
} gq_switch_job_t;

int gq_level_switch(const gq_switch_job_t* jobs_host, int n_jobs, void* stream);

#ifdef __cplusplus
}
#endif
#endif
