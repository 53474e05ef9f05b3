// gq_quadform_core.hpp -- the tile of K17 / K31: one 128 x 128 tile of
//   sum_r d_r H~ d_r^T,   d = f32(A) - f32(B)  (or f32(A) when B is NULL),   A, B [R, C],  H [C, C] fp32 symmetric,
// H~ = H with every exactly-zero diagonal entry read as 1 (evopress/src/error_estimator.py:88-89; H itself is not written),
// as one text that gq_quadform.hip (one matrix) and gq_quad_form_experts.hip (E matrices, E Hessians) both compile, and the
// fixed-order sum of a matrix's tile partials.  The two kernels differ only in how a workgroup finds its operands and its
// slot of the workspace, so that the grouped call is bit for bit the single one.
//
// The GEMM is gq_gemm32.hpp's: v_mfma_f32_32x32x2_f32, 128 x 128 tiles, 4 waves (2 x 2, wave tile 64 x 64), K in chunks of
// 32 through the double-buffered LDS image G32<128> with the commit of chunk t + 1 at G32_COMMIT_AT inside the MFMA block of
// chunk t -- the loop of gemm32_tile<false, 1, false, 1, 0, 128> (NN, k < n0 + 128) with two things that kernel cannot take
// as arguments: the A operand is formed on load (two 16-bit or fp32 reads, one fp32 subtraction) and the epilogue does not
// store the accumulators but multiplies them by the matching d tile and reduces.
//
// Symmetry: tile (row block i, column block j) runs k over column blocks <= j only.  sum_{k, c} d_k H_kc d_c counts every
// off-diagonal block pair twice, so the accumulators are doubled ONCE, exactly, when the k loop reaches the diagonal block,
// which is then taken whole: R C^2 flops instead of 2 R C^2.
//
// No float atomics.  A lane multiplies its 64 accumulators by d in fp32 and adds the products in fp64; lanes merge by an
// xor butterfly, waves through LDS in wave order, and thread 0 holds the tile's fp64 partial.
#pragma once
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

// Tile (row block bi, column block bj) of one matrix; the whole workgroup calls it, the value is the tile's partial on
// thread 0 (other threads: unspecified).  qf_smem: G32<QF_TS>::LDS_BYTES of dynamic LDS.
template <int DTA, int DTB, bool HAS_B>
__device__ __forceinline__ double qf_tile(const typename Ld4<DTA>::E* __restrict__ A, int64_t lda,
                                          const typename Ld4<DTB>::E* __restrict__ B, int64_t ldb,
                                          const float* __restrict__ H, int64_t R, int64_t C, unsigned bi, unsigned bj,
                                          float* qf_smem) {
    constexpr int TS = QF_TS, NV = QF_NV, NT = QF_NT;
    constexpr int WTM = 64, WTN = 64, NIM = 2, NIN = 2;
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
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// part[0 .. n) in a fixed order: thread t takes t, t + 256, ..; lanes by the butterfly, waves in wave order.  The whole
// workgroup (QF_NT threads) calls it; the sum is on thread 0.
__device__ __forceinline__ double qf_sum_partials(const double* __restrict__ part, int64_t n) {
    __shared__ double red[QF_NT / 64];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int64_t i = tid; i < n; i += QF_NT) s += part[i];
    s = qf_wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

inline size_t qf_esize(int dt) { return dt == GQ_F32 ? 4 : 2; }
inline bool qf_dtype_ok(int dt) { return dt == GQ_F32 || dt == GQ_F16 || dt == GQ_BF16; }
inline bool qf_rows_aligned(const void* p, int64_t ld, int dt) {
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (((uint64_t)ld * qf_esize(dt)) & 15) == 0;
}
inline int64_t qf_row_tiles(int64_t R) { return (R + QF_TS - 1) / QF_TS; }
inline int64_t qf_n_tiles(int64_t R, int64_t C) { return qf_row_tiles(R) * (C / QF_TS); }

}  // namespace
}  // namespace gq
