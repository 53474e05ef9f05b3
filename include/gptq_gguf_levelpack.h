/* gptq_gguf_levelpack.h -- the level database straight from the one-pass level build: an additive extension of the C ABI
   of gptq_gguf.h (same library, same conventions: status codes, gq_last_error, device pointers, `stream` a hipStream_t).
   GQ_ABI_VERSION does not change.  The symbol lives in a header of its own so that gptq_gguf.h stays the symbol set its
   version names. */
#ifndef GPTQ_GGUF_LEVELPACK_H
#define GPTQ_GGUF_LEVELPACK_H

#include "gptq_gguf_levels.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the outputs of one gq_gptq_quantize_bands call as GGUF block bytes, every band into a buffer of its own, ONE launch.

   What the bit-width search, the error estimator and the stitcher read of a level is its packed GGUF blocks.  When a walk
   ends, its bands -- the levels of the Linears that share U -- lie on the device; this call packs all of them where their
   consumers want them, with the HF -> GGUF row order of attn_q / attn_k applied as a row gather while the rows are read.

     qweight  [R, C] bytes, d, dmin [R, C / 256] fp16 bit patterns, s, m in the concatenated per-band layout: the outputs of
              gq_gptq_quantize_bands, as that call leaves them (gptq_gguf_levels.h).  All const.  dmin / m are not read for
              Q3_K / Q6_K bands (and may be NULL when the table holds no other type).
     bands    the HOST table of that call: row_end ascending, every row_end % 64 == 0, the last one == R, 1 <= n_bands <=
              GQ_BANDS_MAX, q_type GQ_Q2_K .. GQ_Q6_K; a type may repeat.  Read during the call (it travels in the kernel
              arguments: no staging copy is put on the stream).
     outs     HOST array of n_bands DEVICE pointers: outs[k] receives band k's [rows_k, C / 256 * type_size_k] bytes.
              Every outs[k] must be non-NULL and GQ_PACK_BANDS_ALIGN (16) bytes aligned: a workgroup stores 16 bytes at a
              time from the buffer's base on, as gq_pack does.  The buffers must not overlap each other or the inputs.
     row_srcs HOST array of n_bands DEVICE pointers or NULL (no gather at all): row_srcs[k] is NULL or int32 [rows_k],
              output row r of band k is packed from band row row_srcs[k][r].  Indices are relative to the band, must lie
              in [0, rows_k) and are trusted -- the kernel does not check, as gq_dequantize_blocks does not.

   Contract (exact class): band k's bytes are bit-identical to gq_pack(type_k, ...) on that band's rows alone after those
   rows -- of all five tensors -- were gathered with row_srcs[k].  The +4 / +32 offsets of Q3_K / Q6_K are applied on the
   fly, as gq_pack applies them.

   GQ_E_NULL for a NULL input, table, outs or outs[k]; GQ_E_BAD_SHAPE for a bad table (the rules above), C % 256 != 0, a
   misaligned outs[k] or row_srcs[k]; GQ_E_BAD_TYPE for an unknown type; each with a gq_last_error text.  Every check is
   made before the first HIP call: a refused call has launched nothing and written nothing.  The call only enqueues. */
#define GQ_PACK_BANDS_ALIGN 16

int gq_pack_bands(const uint8_t* qweight, const uint16_t* d, const uint8_t* s, const uint16_t* dmin, const uint8_t* m,
                  int64_t R, int64_t C, const gq_band_t* bands_host, int n_bands, void* const* outs_host,
                  const int32_t* const* row_srcs_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif
