// gq_quad_form_experts.hip -- K31: the calibration-weighted errors of the E experts of a stacked [E, R, C] tensor, each
// with its own Hessian, in two launches whatever E:
//   out[e] = sum_r d_r H~_e d_r^T,   d = f32(A_e) - f32(B_e)  (or f32(A_e) when B is NULL),   H [E, C, C] fp32.
// out[e] is bit for bit gq_quad_form on expert e's operands: the tile is the same text (gq_quadform_core.hpp's qf_tile),
// expert e's partials lie at ws[e * tiles + t] with t the single call's tile number, and quad_sum_experts_kernel adds them
// per expert (one workgroup each) with the single call's qf_sum_partials.  No atomics; every partial is written before it
// is read, so ws contents on entry do not matter.
//
// Tile order: the cost ordering of gq_quad_form's launch, across experts -- deepest column block first, within a column
// block all experts, within an expert its row tiles (neighbours read the same panel of the same H_e).  The long tiles of
// all experts start first and the 1-deep ones fill the tail.
#include "../../../include/gptq_gguf_moe_errest.h"
#include "gq_quadform_core.hpp"

namespace gq {
namespace {

template <int DTA, int DTB, bool HAS_B>
__global__ __launch_bounds__(QF_NT, 2) void quad_form_experts_kernel(const typename Ld4<DTA>::E* __restrict__ A, int64_t lda,
                                                                     int64_t a_stride,
                                                                     const typename Ld4<DTB>::E* __restrict__ B, int64_t ldb,
                                                                     int64_t b_stride, const float* __restrict__ H, unsigned E,
                                                                     int64_t R, int64_t C, unsigned ntr,
                                                                     double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float qf_smem[];
    const unsigned nb = (unsigned)(C / QF_TS);
    const unsigned per_cb = E * ntr;  // tiles of one column block: < 2^31 with the whole grid
    const unsigned cb = blockIdx.x / per_cb, rem = blockIdx.x % per_cb;
    const unsigned e = rem / ntr, bi = rem % ntr, bj = nb - 1 - cb;
    const typename Ld4<DTA>::E* Ae = A + (int64_t)e * a_stride;
    const typename Ld4<DTB>::E* Be = HAS_B ? B + (int64_t)e * b_stride : B;
    const double s = qf_tile<DTA, DTB, HAS_B>(Ae, lda, Be, ldb, H + (int64_t)e * C * C, R, C, bi, bj, qf_smem);
    // slot: expert e's row of partials, at the single call's tile number
    if (threadIdx.x == 0) part[(int64_t)e * nb * ntr + (int64_t)cb * ntr + bi] = s;
}

__global__ __launch_bounds__(QF_NT) void quad_sum_experts_kernel(const double* __restrict__ part, int64_t tiles,
                                                                 double* __restrict__ out) {
    const double s = qf_sum_partials(part + (int64_t)blockIdx.x * tiles, tiles);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

template <int DTA, int DTB, bool HAS_B>
int launch(const void* A, int64_t lda, int64_t a_stride, const void* B, int64_t ldb, int64_t b_stride, const float* H,
           int64_t E, int64_t R, int64_t C, double* part, hipStream_t st) {
    auto* kern = quad_form_experts_kernel<DTA, DTB, HAS_B>;
    static std::atomic<bool> attr_set{false};  // guards an idempotent call: a race sets the same value twice
    if (!attr_set) {
        GQ_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, G32<QF_TS>::LDS_BYTES));
        attr_set = true;
    }
    const unsigned ntr = (unsigned)qf_row_tiles(R);
    hipLaunchKernelGGL(kern, dim3((unsigned)(E * qf_n_tiles(R, C))), dim3(QF_NT), G32<QF_TS>::LDS_BYTES, st,
                       (const typename Ld4<DTA>::E*)A, lda, a_stride, (const typename Ld4<DTB>::E*)B, ldb, b_stride, H,
                       (unsigned)E, R, C, ntr, part);
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

template <int DTA>
int launch_a(const void* A, int64_t lda, int64_t a_stride, const void* B, int b_dtype, int64_t ldb, int64_t b_stride,
             const float* H, int64_t E, int64_t R, int64_t C, double* part, hipStream_t st) {
    if (!B) return launch<DTA, DTA, false>(A, lda, a_stride, nullptr, 0, 0, H, E, R, C, part, st);
    switch (b_dtype) {
    case GQ_F32: return launch<DTA, GQ_F32, true>(A, lda, a_stride, B, ldb, b_stride, H, E, R, C, part, st);
    case GQ_F16: return launch<DTA, GQ_F16, true>(A, lda, a_stride, B, ldb, b_stride, H, E, R, C, part, st);
    default: return launch<DTA, GQ_BF16, true>(A, lda, a_stride, B, ldb, b_stride, H, E, R, C, part, st);
    }
}

// expert e's matrix starts at + e * stride elements: 16-byte aligned like the first, and behind the matrix before it
bool stride_ok(int64_t stride, int64_t ld, int64_t E, int64_t R, int64_t C, int dt) {
    if (E == 1) return true;
    return stride >= (R - 1) * ld + C && (((uint64_t)stride * qf_esize(dt)) & 15) == 0;
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

size_t gq_quad_form_experts_workspace_bytes(int64_t E, int64_t R, int64_t C) {
    if (E < 1 || E > GQ_QUAD_EXPERTS_MAX || R < 1 || C < QF_TS || C % QF_TS) return 0;
    return (size_t)E * (size_t)qf_n_tiles(R, C) * sizeof(double);
}

int gq_quad_form_experts(const void* A, int a_dtype, int64_t lda, int64_t a_stride, const void* B, int b_dtype, int64_t ldb,
                         int64_t b_stride, const float* H, int64_t E, int64_t R, int64_t C, double* out, void* ws,
                         size_t ws_bytes, void* stream) {
    if (int rc = options_ok()) return rc;
    if (!A) GQ_FAIL(GQ_E_NULL, "gq_quad_form_experts: A is NULL");
    if (!H) GQ_FAIL(GQ_E_NULL, "gq_quad_form_experts: H is NULL");
    if (!out) GQ_FAIL(GQ_E_NULL, "gq_quad_form_experts: out is NULL");
    if (!qf_dtype_ok(a_dtype)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_quad_form_experts: unknown a_dtype %d", a_dtype);
    if (B && !qf_dtype_ok(b_dtype)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_quad_form_experts: unknown b_dtype %d", b_dtype);
    if (E < 1 || E > GQ_QUAD_EXPERTS_MAX)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form_experts: E=%ld is not in 1 .. %d", (long)E, GQ_QUAD_EXPERTS_MAX);
    if (R < 1) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form_experts: R=%ld must be positive", (long)R);
    if (C < QF_TS || C % QF_TS)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form_experts: C=%ld is not a positive multiple of %d", (long)C, QF_TS);
    if (qf_n_tiles(R, C) > 0x7fffffffLL / E)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form_experts: E=%ld x R=%ld x C=%ld has more than 2^31 tiles", (long)E, (long)R, (long)C);
    if (lda < C) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form_experts: lda=%ld is smaller than C=%ld", (long)lda, (long)C);
    if (B && ldb < C) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form_experts: ldb=%ld is smaller than C=%ld", (long)ldb, (long)C);
    if (!qf_rows_aligned(A, lda, a_dtype))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form_experts: the rows of A are not 16-byte aligned (pointer and lda * element size)");
    if (B && !qf_rows_aligned(B, ldb, b_dtype))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form_experts: the rows of B are not 16-byte aligned (pointer and ldb * element size)");
    if (!stride_ok(a_stride, lda, E, R, C, a_dtype))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form_experts: a_stride=%ld must be a multiple of 16 bytes and at least (R - 1) * lda + C = %ld elements",
                (long)a_stride, (long)((R - 1) * lda + C));
    if (B && !stride_ok(b_stride, ldb, E, R, C, b_dtype))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form_experts: b_stride=%ld must be a multiple of 16 bytes and at least (R - 1) * ldb + C = %ld elements",
                (long)b_stride, (long)((R - 1) * ldb + C));
    if (reinterpret_cast<uintptr_t>(H) & 15) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form_experts: H is not 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(out) & 7) || (reinterpret_cast<uintptr_t>(ws) & 7))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form_experts: out / ws are not 8-byte aligned");
    const size_t need = gq_quad_form_experts_workspace_bytes(E, R, C);
    if (!ws || ws_bytes < need) GQ_FAIL(GQ_E_WORKSPACE, "gq_quad_form_experts: workspace %zu < %zu bytes", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(ws);
    int rc;
    switch (a_dtype) {
    case GQ_F32: rc = launch_a<GQ_F32>(A, lda, a_stride, B, b_dtype, ldb, b_stride, H, E, R, C, part, st); break;
    case GQ_F16: rc = launch_a<GQ_F16>(A, lda, a_stride, B, b_dtype, ldb, b_stride, H, E, R, C, part, st); break;
    default: rc = launch_a<GQ_BF16>(A, lda, a_stride, B, b_dtype, ldb, b_stride, H, E, R, C, part, st); break;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(quad_sum_experts_kernel, dim3((unsigned)E), dim3(QF_NT), 0, st, (const double*)part, qf_n_tiles(R, C), out);
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
