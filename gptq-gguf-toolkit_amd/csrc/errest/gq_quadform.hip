// gq_quadform.hip -- K17: the calibration-weighted error of a compressed Linear,
//   out[0] = sum_r d_r H~ d_r^T,   d = f32(A) - f32(B)  (or f32(A) when B is NULL),   A, B [R, C],  H [C, C] fp32 symmetric,
// H~ = H with every exactly-zero diagonal entry read as 1 (evopress/src/error_estimator.py:88-89; H itself is not written).
// Numerator and denominator of error_estimator.py:101-102 are one call each; the [R, C] product D @ H, D itself and the
// elementwise product never exist in memory.
//
// The tile (GEMM, symmetry, fp64 reduction) is gq_quadform_core.hpp's qf_tile.  Tile cost grows with the column block j:
// the launch is one-dimensional and lists the column blocks from the last (C / 128 chunks-of-128 deep) to the first, row
// tiles of one column block next to each other (they read the same panel of H), so the deepest tiles start first and the
// 1-deep ones fill the tail.
//
// The tile's fp64 partial goes to ws[tile].  quad_sum_kernel (one workgroup) adds the partials in a fixed order.  Every
// partial is written before it is read: ws contents on entry do not matter, and the result is a function of
// (A, B, H, R, C) alone.
#include "../../../include/gptq_gguf_errest.h"
#include "gq_quadform_core.hpp"

namespace gq {
namespace {

template <int DTA, int DTB, bool HAS_B>
__global__ __launch_bounds__(QF_NT, 2) void quad_form_kernel(const typename Ld4<DTA>::E* __restrict__ A, int64_t lda,
                                                             const typename Ld4<DTB>::E* __restrict__ B, int64_t ldb,
                                                             const float* __restrict__ H, int64_t R, int64_t C, unsigned ntr,
                                                             double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float qf_smem[];
    const unsigned nb = (unsigned)(C / QF_TS);
    // deepest column blocks first; the row tiles of one column block are neighbours
    const unsigned bj = nb - 1 - blockIdx.x / ntr, bi = blockIdx.x % ntr;
    const double s = qf_tile<DTA, DTB, HAS_B>(A, lda, B, ldb, H, R, C, bi, bj, qf_smem);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(QF_NT) void quad_sum_kernel(const double* __restrict__ part, int64_t n, double* __restrict__ out) {
    const double s = qf_sum_partials(part, n);
    if (threadIdx.x == 0) out[0] = s;
}

template <int DTA, int DTB, bool HAS_B>
int launch(const void* A, int64_t lda, const void* B, int64_t ldb, const float* H, int64_t R, int64_t C, double* part,
           hipStream_t st) {
    auto* kern = quad_form_kernel<DTA, DTB, HAS_B>;
    static std::atomic<bool> attr_set{false};  // guards an idempotent call: a race sets the same value twice
    if (!attr_set) {
        GQ_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, G32<QF_TS>::LDS_BYTES));
        attr_set = true;
    }
    const unsigned ntr = (unsigned)qf_row_tiles(R);
    hipLaunchKernelGGL(kern, dim3((unsigned)qf_n_tiles(R, C)), dim3(QF_NT), G32<QF_TS>::LDS_BYTES, st,
                       (const typename Ld4<DTA>::E*)A, lda, (const typename Ld4<DTB>::E*)B, ldb, H, R, C, ntr, part);
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

template <int DTA>
int launch_a(const void* A, int64_t lda, const void* B, int b_dtype, int64_t ldb, const float* H, int64_t R, int64_t C,
             double* part, hipStream_t st) {
    if (!B) return launch<DTA, DTA, false>(A, lda, nullptr, 0, H, R, C, part, st);
    switch (b_dtype) {
    case GQ_F32: return launch<DTA, GQ_F32, true>(A, lda, B, ldb, H, R, C, part, st);
    case GQ_F16: return launch<DTA, GQ_F16, true>(A, lda, B, ldb, H, R, C, part, st);
    default: return launch<DTA, GQ_BF16, true>(A, lda, B, ldb, H, R, C, part, st);
    }
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

size_t gq_quad_form_workspace_bytes(int64_t R, int64_t C) {
    if (R < 1 || C < QF_TS || C % QF_TS) return 0;
    return (size_t)qf_n_tiles(R, C) * sizeof(double);
}

int gq_quad_form(const void* A, int a_dtype, int64_t lda, const void* B, int b_dtype, int64_t ldb, const float* H, int64_t R,
                 int64_t C, double* out, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = options_ok()) return rc;
    if (!A) GQ_FAIL(GQ_E_NULL, "gq_quad_form: A is NULL");
    if (!H) GQ_FAIL(GQ_E_NULL, "gq_quad_form: H is NULL");
    if (!out) GQ_FAIL(GQ_E_NULL, "gq_quad_form: out is NULL");
    if (!qf_dtype_ok(a_dtype)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_quad_form: unknown a_dtype %d", a_dtype);
    if (B && !qf_dtype_ok(b_dtype)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_quad_form: unknown b_dtype %d", b_dtype);
    if (R < 1) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form: R=%ld must be positive", (long)R);
    if (C < QF_TS || C % QF_TS) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form: C=%ld is not a positive multiple of %d", (long)C, QF_TS);
    if (qf_n_tiles(R, C) > 0x7fffffffLL) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form: R=%ld x C=%ld has more than 2^31 tiles", (long)R, (long)C);
    if (lda < C) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form: lda=%ld is smaller than C=%ld", (long)lda, (long)C);
    if (B && ldb < C) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form: ldb=%ld is smaller than C=%ld", (long)ldb, (long)C);
    if (!qf_rows_aligned(A, lda, a_dtype)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form: the rows of A are not 16-byte aligned (pointer and lda * element size)");
    if (B && !qf_rows_aligned(B, ldb, b_dtype)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form: the rows of B are not 16-byte aligned (pointer and ldb * element size)");
    if (reinterpret_cast<uintptr_t>(H) & 15) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form: H is not 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(out) & 7) || (reinterpret_cast<uintptr_t>(ws) & 7))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form: out / ws are not 8-byte aligned");
    const size_t need = gq_quad_form_workspace_bytes(R, C);
    if (!ws || ws_bytes < need) GQ_FAIL(GQ_E_WORKSPACE, "gq_quad_form: workspace %zu < %zu bytes", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(ws);
    int rc;
    switch (a_dtype) {
    case GQ_F32: rc = launch_a<GQ_F32>(A, lda, B, b_dtype, ldb, H, R, C, part, st); break;
    case GQ_F16: rc = launch_a<GQ_F16>(A, lda, B, b_dtype, ldb, H, R, C, part, st); break;
    default: rc = launch_a<GQ_BF16>(A, lda, B, b_dtype, ldb, H, R, C, part, st); break;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(quad_sum_kernel, dim3(1), dim3(QF_NT), 0, st, (const double*)part, qf_n_tiles(R, C), out);
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
