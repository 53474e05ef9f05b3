/* gptq_gguf_moe_errest.h -- the layer error estimate of a stacked expert tensor: an additive extension of the C ABI of
   gptq_gguf.h (same library, same conventions: status codes, gq_last_error, GQ_F32 / GQ_F16 / GQ_BF16, device pointers,
   `stream` a hipStream_t).  GQ_ABI_VERSION does not change.  The two symbols live in a header of their own so that
   gptq_gguf.h stays the symbol set its version names. */
#ifndef GPTQ_GGUF_MOE_ERREST_H
#define GPTQ_GGUF_MOE_ERREST_H

#include "gptq_gguf_errest.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_QUAD_EXPERTS_MAX 256 /* experts of one gq_quad_form_experts call */

/* ---- gq_quad_form for the E experts of a unit, each with its own Hessian, in two launches whatever E:
     out[e] = sum_r d_r H~_e d_r^T,   d = f32(A_e) - f32(B_e), one fp32 subtraction on load;   d = f32(A_e) when B is NULL.
   A_e = A + e * a_stride, B_e = B + e * b_stride (strides in ELEMENTS of the operand's dtype), each an [R, C] matrix as
   gq_quad_form reads it: row r at + r * ld elements, rows 16-byte aligned (the pointer, ld * element size and, for E > 1,
   stride * element size); stride >= (R - 1) * ld + C for E > 1 and otherwise free, so both halves of a fused
   gate_up_proj [E, 2 I, H] are read in place with a_stride = 2 I H.  H: [E, C, C] fp32, contiguous, 16-byte aligned,
   H_e = H + e * C * C SYMMETRIC; H~_e is H_e with every exactly-zero diagonal entry read as 1, so an all-zero H_e (an
   expert no calibration token reached) is the identity.  H is not written.
   1 <= E <= GQ_QUAD_EXPERTS_MAX, R >= 1, C % 128 == 0, E * tiles(R, C) < 2^31 (tiles = ceil(R / 128) * C / 128); anything
   else is GQ_E_BAD_SHAPE.  Every refusal is raised before the first HIP call.
   out[e] is BIT FOR BIT what gq_quad_form writes for expert e's operands: the same tile, the same fp64 order inside a
   tile, the same fixed-order sum over the expert's tile partials, which lie at ws[e * tiles + t], t the single call's tile
   number.  No atomics.  out: E doubles on the device.  ws: gq_quad_form_experts_workspace_bytes(E, R, C) bytes (0 for
   arguments the call refuses), 8-byte aligned, contents on entry irrelevant.  The call only enqueues. */
size_t gq_quad_form_experts_workspace_bytes(int64_t E, int64_t R, int64_t C);
int gq_quad_form_experts(const void* A, int a_dtype, int64_t lda, int64_t a_stride,
                         const void* B, int b_dtype, int64_t ldb, int64_t b_stride, /* B may be NULL */
                         const float* H,                                           /* [E, C, C] fp32, contiguous */
                         int64_t E, int64_t R, int64_t C,
                         double* out, /* [E] on the device */
                         void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
