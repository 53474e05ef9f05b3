// gq_quadform.hip -- K17: the calibration-weighted error of a compressed Linear,
//   out[0] = sum_r d_r H~ d_r^T,   d = f32(A) - f32(B)  (or f32(A) when B is NULL),   A, B [R, C],  H [C, C] fp32 symmetric,
// H~ = H with every exactly-zero diagonal entry read as 1 (evopress/src/error_estimator.py:88-89; H itself is not written).
// Numerator and denominator of error_estimator.py:101-102 are one call each; the [R, C] product D @ H, D itself and the
// elementwise product never exist in memory.
//
// The GEMM is gq_gemm32.hpp's: v_mfma_f32_32x32x2_f32, 128 x 128 tiles, 4 waves (2 x 2, wave tile 64 x 64), K in chunks of
// 32 through the double-buffered LDS image G32<128> with the commit of chunk t + 1 at G32_COMMIT_AT inside the MFMA block of
// chunk t -- the loop of gemm32_tile<false, 1, false, 1, 0, 128> (NN, k < n0 + 128) with two things that kernel cannot take
// as arguments: the A operand is formed on load (two 16-bit or fp32 reads, one fp32 subtraction) and the epilogue does not
// store the accumulators but multiplies them by the matching d tile and reduces.
//
// Symmetry: tile (row block i, column block j) runs k over column blocks <= j only.  sum_{k, c} d_k H_kc d_c counts every
// off-diagonal block pair twice, so the accumulators are doubled ONCE, exactly, when the k loop reaches the diagonal block,
// which is then taken whole: R C^2 flops instead of 2 R C^2.  Tile cost grows with j: the launch is one-dimensional and
// lists the column blocks from the last (C / 128 chunks-of-128 deep) to the first, row tiles of one column block next to
// each other (they read the same panel of H), so the deepest tiles start first and the 1-deep ones fill the tail.
//
// No float atomics.  A lane multiplies its 64 accumulators by d in fp32 and adds the products in fp64; lanes merge by an
// xor butterfly, waves through LDS in wave order, and the tile's fp64 partial goes to ws[tile].  quad_sum_kernel (one
// workgroup) adds the partials in a fixed order.  Every partial is written before it is read: ws contents on entry do not
// matter, and the result is a function of (A, B, H, R, C) alone.
#include "../../../include/gptq_gguf_errest.h"
#include "../gq_common.hpp"
#include "../gq_gemm32.hpp"

namespace gq {
namespace {

constexpr int QF_TS = 128, QF_NT = 256, QF_NV = 4;

// 4 consecutive elements of a row (16-byte aligned rows, offsets multiples of 4 elements) as fp32
template <int DT> struct Ld4;
template <> struct Ld4<GQ_F32> {
    using E = float;
    static __device__ __forceinline__ float one(const E* p) { return *p; }
    static __device__ __forceinline__ float4 four(const E* p) { return *reinterpret_cast<const float4*>(p); }
};
template <> struct Ld4<GQ_F16> {
    using E = uint16_t;
    static __device__ __forceinline__ float one(const E* p) { return h2f(*p); }
    static __device__ __forceinline__ float4 four(const E* p) {
        const uint2 w = *reinterpret_cast<const uint2*>(p);
        return make_float4(h2f((uint16_t)(w.x & 0xffffu)), h2f((uint16_t)(w.x >> 16)), h2f((uint16_t)(w.y & 0xffffu)),
                           h2f((uint16_t)(w.y >> 16)));
    }
};
template <> struct Ld4<GQ_BF16> {
    using E = uint16_t;
    static __device__ __forceinline__ float one(const E* p) { return bf2f(*p); }
    static __device__ __forceinline__ float4 four(const E* p) {
        const uint2 w = *reinterpret_cast<const uint2*>(p);
        return make_float4(__builtin_bit_cast(float, w.x << 16), __builtin_bit_cast(float, w.x & 0xffff0000u),
                           __builtin_bit_cast(float, w.y << 16), __builtin_bit_cast(float, w.y & 0xffff0000u));
    }
};

// the d chunk [128 rows][32 k] in the thread mapping of g32_load_rows (row = idx >> 3, 4 k at (idx & 7) * 4); rows >= R are 0
template <int DTA, int DTB, bool HAS_B>
__device__ __forceinline__ void qf_load_d(float4 (&v)[QF_NV], const typename Ld4<DTA>::E* A, int64_t lda,
                                          const typename Ld4<DTB>::E* B, int64_t ldb, int64_t m0, int64_t R, int64_t k0, int tid) {
#pragma unroll
    for (int t = 0; t < QF_NV; ++t) {
        const int idx = tid + t * QF_NT, rr = idx >> 3, c4 = (idx & 7) * 4;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m0 + rr < R) {
            x = Ld4<DTA>::four(A + (m0 + rr) * lda + k0 + c4);
            if constexpr (HAS_B) {
                const float4 y = Ld4<DTB>::four(B + (m0 + rr) * ldb + k0 + c4);
                x.x = x.x - y.x; x.y = x.y - y.y; x.z = x.z - y.z; x.w = x.w - y.w;
            }
        }
        v[t].x = x.x; v[t].y = x.y; v[t].z = x.z; v[t].w = x.w;
    }
}

// the H chunk [32 k][128 columns] in the thread mapping of g32_load_kn_full (k = idx / 32, 4 columns at (idx % 32) * 4),
// a zero on the diagonal of H read as 1
__device__ __forceinline__ void qf_load_h(float4 (&v)[QF_NV], const float* H, int64_t C, int64_t n0, int64_t k0, int tid) {
    g32_load_kn_full<QF_NV, QF_NT>(v, H, C, n0, k0, tid);
#pragma unroll
    for (int t = 0; t < QF_NV; ++t) {
        const int idx = tid + t * QF_NT, kk = idx >> 5, c4 = (idx & 31) * 4;
        const int64_t dg = k0 + kk - n0 - c4;  // the component of v[t] that lies on the diagonal, if in [0, 4)
        v[t].x = (dg == 0 && v[t].x == 0.f) ? 1.f : v[t].x;
        v[t].y = (dg == 1 && v[t].y == 0.f) ? 1.f : v[t].y;
        v[t].z = (dg == 2 && v[t].z == 0.f) ? 1.f : v[t].z;
        v[t].w = (dg == 3 && v[t].w == 0.f) ? 1.f : v[t].w;
    }
}

__device__ __forceinline__ double qf_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

template <int DTA, int DTB, bool HAS_B>
__global__ __launch_bounds__(QF_NT, 2) void quad_form_kernel(const typename Ld4<DTA>::E* __restrict__ A, int64_t lda,
                                                             const typename Ld4<DTB>::E* __restrict__ B, int64_t ldb,
                                                             const float* __restrict__ H, int64_t R, int64_t C, unsigned ntr,
                                                             double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float qf_smem[];
    constexpr int TS = QF_TS, NV = QF_NV, NT = QF_NT;
    constexpr int WTM = 64, WTN = 64, NIM = 2, NIN = 2;
    const unsigned nb = (unsigned)(C / TS);
    // deepest column blocks first; the row tiles of one column block are neighbours
    const unsigned bj = nb - 1 - blockIdx.x / ntr, bi = blockIdx.x % ntr;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int64_t m0 = (int64_t)bi * TS, n0 = (int64_t)bj * TS;
    f32x16 acc[NIM][NIN];
#pragma unroll
    for (int i = 0; i < NIM; ++i)
#pragma unroll
        for (int j = 0; j < NIN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    float4 va[NV], vb[NV];
    auto fetch = [&](int64_t k0) {
        qf_load_d<DTA, DTB, HAS_B>(va, A, lda, B, ldb, m0, R, k0, tid);
        qf_load_h(vb, H, C, n0, k0, tid);
    };
    auto commit = [&](int buf) {
        float* As = qf_smem + buf * G32<TS>::STAGE_FLOATS;
        g32_store_rows<NV, NT>(va, As, LDA_S, tid);
        g32_store_kn<NV, NT>(vb, As + G32<TS>::A_FLOATS, tid);
    };
    const int li = lane & 31, lk = lane >> 5;
    const int64_t nk = (n0 + TS) / TK;  // k < n0 + 128: the column blocks <= j
    const int64_t t_diag = n0 / TK;     // first chunk of the diagonal block
    fetch(0);
    commit(0);
    fetch((nk > 1) ? TK : 0);
    __syncthreads();
    for (int64_t t = 0; t < nk; ++t) {
        const float* As = qf_smem + (t & 1) * G32<TS>::STAGE_FLOATS;
        const float* Bs = As + G32<TS>::A_FLOATS;
        float av[2][NIM], bv[2][NIN];
        auto frag = [&](int kk, float (&a)[NIM], float (&b)[NIN]) {
#pragma unroll
            for (int i = 0; i < NIM; ++i) a[i] = As[(wm * WTM + i * 32 + li) * LDA_S + kk + lk];
#pragma unroll
            for (int j = 0; j < NIN; ++j) b[j] = Bs[(kk + lk) * G32<TS>::LDB + wn * WTN + j * 32 + li];
        };
        frag(0, av[0], bv[0]);
#pragma unroll
        for (int kk = 0; kk < TK; kk += 2) {
            const int cur = (kk >> 1) & 1;
            if (kk + 2 < TK) frag(kk + 2, av[cur ^ 1], bv[cur ^ 1]);
            if (kk == G32_COMMIT_AT) {
                // unconditional (one basic block per chunk): past the end the last chunk is fetched again and
                // committed to the buffer nobody reads
                commit((int)((t + 1) & 1));
                fetch(((t + 2 < nk) ? t + 2 : nk - 1) * TK);
            }
#pragma unroll
            for (int i = 0; i < NIM; ++i)
#pragma unroll
                for (int j = 0; j < NIN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cur][i], bv[cur][j], acc[i][j], 0, 0, 0);
        }
        if (t + 1 == t_diag) {  // everything so far lies above the diagonal block: weight 2 (exact)
#pragma unroll
            for (int i = 0; i < NIM; ++i)
#pragma unroll
                for (int j = 0; j < NIN; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][j][e] = acc[i][j][e] * 2.0f;
        }
        __syncthreads();
    }
    // D layout: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5).  Products in fp32, their sum in fp64.
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NIM; ++i)
#pragma unroll
        for (int j = 0; j < NIN; ++j) {
            const int64_t col = n0 + wn * WTN + j * 32 + li;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int64_t rowi = m0 + wm * WTM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lk;
                if (rowi < R) {
                    float d = Ld4<DTA>::one(A + rowi * lda + col);
                    if constexpr (HAS_B) d = d - Ld4<DTB>::one(B + rowi * ldb + col);
                    s += (double)(acc[i][j][e] * d);
                }
            }
        }
    s = qf_wave_sum(s);
    double* red = reinterpret_cast<double*>(qf_smem);  // free: every wave passed the barrier behind the last chunk
    if (lane == 0) red[wid] = s;
    __syncthreads();
    if (tid == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(QF_NT) void quad_sum_kernel(const double* __restrict__ part, int64_t n, double* __restrict__ out) {
    __shared__ double red[QF_NT / 64];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int64_t i = tid; i < n; i += QF_NT) s += part[i];
    s = qf_wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) out[0] = ((red[0] + red[1]) + red[2]) + red[3];
}

size_t esize(int dt) { return dt == GQ_F32 ? 4 : 2; }
bool dtype_ok(int dt) { return dt == GQ_F32 || dt == GQ_F16 || dt == GQ_BF16; }
bool rows_aligned(const void* p, int64_t ld, int dt) {
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (((uint64_t)ld * esize(dt)) & 15) == 0;
}
int64_t n_tiles(int64_t R, int64_t C) { return ((R + QF_TS - 1) / QF_TS) * (C / QF_TS); }

template <int DTA, int DTB, bool HAS_B>
int launch(const void* A, int64_t lda, const void* B, int64_t ldb, const float* H, int64_t R, int64_t C, double* part,
           hipStream_t st) {
    auto* kern = quad_form_kernel<DTA, DTB, HAS_B>;
    static std::atomic<bool> attr_set{false};  // guards an idempotent call: a race sets the same value twice
    if (!attr_set) {
        GQ_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, G32<QF_TS>::LDS_BYTES));
        attr_set = true;
    }
    const unsigned ntr = (unsigned)((R + QF_TS - 1) / QF_TS);
    hipLaunchKernelGGL(kern, dim3((unsigned)n_tiles(R, C)), dim3(QF_NT), G32<QF_TS>::LDS_BYTES, st,
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
    return (size_t)n_tiles(R, C) * sizeof(double);
}

int gq_quad_form(const void* A, int a_dtype, int64_t lda, const void* B, int b_dtype, int64_t ldb, const float* H, int64_t R,
                 int64_t C, double* out, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = options_ok()) return rc;
    if (!A) GQ_FAIL(GQ_E_NULL, "gq_quad_form: A is NULL");
    if (!H) GQ_FAIL(GQ_E_NULL, "gq_quad_form: H is NULL");
    if (!out) GQ_FAIL(GQ_E_NULL, "gq_quad_form: out is NULL");
    if (!dtype_ok(a_dtype)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_quad_form: unknown a_dtype %d", a_dtype);
    if (B && !dtype_ok(b_dtype)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_quad_form: unknown b_dtype %d", b_dtype);
    if (R < 1) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form: R=%ld must be positive", (long)R);
    if (C < QF_TS || C % QF_TS) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form: C=%ld is not a positive multiple of %d", (long)C, QF_TS);
    if (n_tiles(R, C) > 0x7fffffffLL) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form: R=%ld x C=%ld has more than 2^31 tiles", (long)R, (long)C);
    if (lda < C) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form: lda=%ld is smaller than C=%ld", (long)lda, (long)C);
    if (B && ldb < C) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form: ldb=%ld is smaller than C=%ld", (long)ldb, (long)C);
    if (!rows_aligned(A, lda, a_dtype)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form: the rows of A are not 16-byte aligned (pointer and lda * element size)");
    if (B && !rows_aligned(B, ldb, b_dtype)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quad_form: the rows of B are not 16-byte aligned (pointer and ldb * element size)");
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
    hipLaunchKernelGGL(quad_sum_kernel, dim3(1), dim3(QF_NT), 0, st, (const double*)part, n_tiles(R, C), out);
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
