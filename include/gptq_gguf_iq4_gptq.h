/* gptq_gguf_iq4_gptq.h -- GPTQ's column walk on the IQ4_XS / IQ4_NL grid, and the packer of its outputs: an additive extension of
   the C ABI of gptq_gguf.h in the way of gptq_gguf_iq4_encode.h (same library, same conventions: status codes, gq_last_error,
   device pointers, `stream` a hipStream_t).  GQ_ABI_VERSION does not change.  The layouts and the decode side are
   gptq_gguf_iq4.h's, the scale search is gptq_gguf_iq4_encode.h's. */
#ifndef GPTQ_GGUF_IQ4_GPTQ_H
#define GPTQ_GGUF_IQ4_GPTQ_H

#include "gptq_gguf_iq4_encode.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the walk: W [R, C] fp32 becomes the dequantized matrix, every rounding error pushed into later columns through U.
     W, U        as gq_gptq_quantize: W contiguous [R, C] fp32, U [C, C] fp32 (the upper Cholesky factor of the inverse Hessian).
     q_type      GQ_IQ4_XS or GQ_IQ4_NL.  C % 256 == 0 for BOTH (the walk's rule), R >= 1.
     block_size  as gq_gptq_quantize (a multiple of 16; <= 0 or > C: C).
     importance  NULL, or C fp32 values on the device, 16-byte aligned, as gq_quantize_iq4.
     qweight     [R, C] uint8, one code 0 .. 15 per byte.
     d, ls       IQ4_XS: d = fp16 bits of D [R, C / 256], ls = 0 .. 63 [R, C / 32].
                 IQ4_NL: d = fp16 bits of d [R, C / 32]; ls is not touched and may be NULL.
     step, istep [R, C / 32] fp32 each, see the contract.
     ws          gq_workspace_bytes(GQ_WS_GPTQ_QUANTIZE, R, C, 0, block_size) bytes: the workspace of the K-quant walk.
   GQ_E_BAD_TYPE for q_type, GQ_E_BAD_SHAPE for the shape rules and the alignment of importance, GQ_E_NULL, GQ_E_UNSUPPORTED for
   a block_size that is no multiple of 16, GQ_E_WORKSPACE; every check is made before the first HIP call.  The call only
   enqueues: no allocation, no host synchronisation.  act_order and static groups do not exist on this grid.

   Contract (exact class), operation by operation; fp32 throughout, no contraction.
   The walk is gptq.py:222-270 as gq_gptq_quantize runs it: the same blocks, the same in-block rank-1 updates, the same
   trailing update.
     in-block:  after column j of a block, for every later column k of the block:  w[k] = w[k] + (-err) * U[j, k]  (the product
                rounded, then the sum: two roundings).
     trailing:  after the block of columns [c1, c2):  W[:, c2:] -= Err @ U[c1:c2, c2:], per element a k-ordered fmaf chain from 0
                over the block's columns and one subtraction.
   Scales.  When the walk reaches a column a with a % 256 == 0, the scales of the columns [a, a + 256) are found by the scale
     search of gptq_gguf_iq4_encode.h, verbatim (sigma2, the weights, the 16 candidates in its order; for IQ4_XS ms, D, l, dl),
     applied to W[:, a : a + 256] as it is in memory at that moment (the global W: with a block_size that does not divide 256 the
     columns of a block under way are stale there by design, as for the K-quants' lazy search) with importance[a : a + 256].
   Per 32-column block and row:
     istep  the encoder's own fp32 inverse: idl (IQ4_XS), id (IQ4_NL); 0 where the encoder uses 0.
     step   what the decoder multiplies by: h2f(f2h(D)) * (ls - 32) (IQ4_XS), h2f(f2h(d)) (IQ4_NL).
   Column j, with w its error-compensated value:
     code = best(istep * w)   (best of gptq_gguf_iq4_encode.h: the two rounded differences, a tie goes up)
     wq   = step * kv[code]   exact in fp32 (11 + 5 + 7 significand bits), written back to W
     err  = (w - wq) / U[j, j], correctly rounded.
   A block with step == 0 comes back as wq == 0 (and with istep == 0, as code 8 everywhere).
   Two consequences, by construction: with U = I the bytes gq_pack_iq4 makes of the outputs are those of gq_quantize_iq4 on the
   same W and importance; and the returned W is exactly what gq_dequantize_blocks makes of the packed bytes (as fp32 values:
   the sign of a zero may differ). */
int gq_gptq_quantize_iq4(float* W, const float* U, int64_t R, int64_t C, int q_type, int block_size, const float* importance,
                         uint8_t* qweight, uint16_t* d, uint8_t* ls, float* step, float* istep, void* ws, size_t ws_bytes,
                         void* stream);

/* ---- the packer: blocks[r, :] = the block bytes of row row_src ? row_src[r] : r of (qweight, d, ls), in the layouts of
   gptq_gguf_iq4.h.  One launch, 16-byte stores; nothing outside [blocks, blocks + R * row bytes) is written.
     q_type   GQ_IQ4_XS (C % 256 == 0) or GQ_IQ4_NL (C % 32 == 0); qweight [R, C], d and ls as above (ls may be NULL for IQ4_NL).
     row_src  NULL (identity) or R int32 row indices on the device, each in [0, R) -- trusted.
     blocks   R * C / 32 * 18 (IQ4_NL) or R * C / 256 * 136 (IQ4_XS) bytes, 16-byte aligned; qweight 16-byte aligned.
   Checks before the first HIP call as above; enqueue-only. */
int gq_pack_iq4(int q_type, int64_t R, int64_t C, const uint8_t* qweight, const uint16_t* d, const uint8_t* ls,
                const int32_t* row_src, uint8_t* blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif
