/* gptq_gguf_errest.h -- the layer error estimate of libgptqgguf_hip.so: an additive extension of the C ABI of
   gptq_gguf.h (same library, same conventions: status codes, gq_last_error, GQ_F32 / GQ_F16 / GQ_BF16, device pointers,
   `stream` a hipStream_t).  GQ_ABI_VERSION does not change.  The two symbols live in a header of their own so that
   gptq_gguf.h stays the symbol set its version names. */
#ifndef GPTQ_GGUF_ERREST_H
#define GPTQ_GGUF_ERREST_H

#include "gptq_gguf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the calibration-weighted error of a compressed Linear (replaces evopress/src/error_estimator.py:88-103: pre_step's
   dead-channel fix and both sums of estimate()):
     out[0] = sum_r d_r H~ d_r^T,   d = f32(A) - f32(B), one fp32 subtraction on load;   d = f32(A) when B is NULL.
   A, B: [R, C] in GQ_F32 / GQ_F16 / GQ_BF16 (each its own dtype), row r at + r * ld elements, rows 16-byte aligned (the
   pointer and ld * element size).  H: [C, C] fp32, contiguous, 16-byte aligned, SYMMETRIC (only blocks on and above the
   block diagonal are read); H~ is H with every exactly-zero diagonal entry read as 1.  H is not written.  C % 128 == 0,
   R >= 1, anything else is GQ_E_BAD_SHAPE.  estimate() is gq_quad_form(W, W_c) / gq_quad_form(W, NULL).
   fp32 MFMA products (R C^2 flops: the symmetric half), fp64 from the first cross-lane sum on, no atomics: the value is a
   function of the operands, not of the launch.  out: one double on the device.  ws: gq_quad_form_workspace_bytes(R, C)
   bytes, 8-byte aligned, contents on entry irrelevant.  The call only enqueues. */
size_t gq_quad_form_workspace_bytes(int64_t R, int64_t C);
int gq_quad_form(const void* A, int a_dtype, int64_t lda, const void* B, int b_dtype, int64_t ldb, const float* H, int64_t R,
                 int64_t C, double* out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
