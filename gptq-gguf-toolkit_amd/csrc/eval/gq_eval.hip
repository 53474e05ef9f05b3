// gq_eval.hip -- K16: the scoring tail of an evaluated sequence.  logits [T, V] -> one fp32 value per row:
//   gq_eval_nll        logsumexp(x) - x[label]                (F.cross_entropy, reduction "none")
//   gq_eval_kl         sum_v p_v (log p_v - log q_v)           (F.kl_div(log_softmax(x), log_softmax(t), log_target=True) per row)
//   gq_eval_kl_sparse  the same over K gathered columns        (logits.gather(-1, ids) first)
//
// HBM-bound streaming, ONE read of every operand and T (or 2 T) floats out.  One workgroup of 256 threads per row.  A row
// starts at logits + t * ld elements, which is 2- or 4-byte aligned only (V = 50257 in fp16: every second row): the lanes
// take the < 16 bytes before the first 16-byte boundary and after the last one as single elements and everything between
// as 16-byte loads; nothing outside [row, row + V) is read.
//
// Online softmax.  A lane keeps (m, S) = (running maximum, sum of e^(x - m)) and rescales S only when a chunk raises m.
// The exponent is (x - m) * log2(e) -- the subtraction first, in the inputs' own scale, so that the terms near the maximum
// (the ones that carry the sum) get an exact exponent -- fed to the hardware exp2 (v_exp_f32).  The dense KL carries five
// values, (m_t, S_t, A = sum e^(t - m_t) (t - x)) for the target and (m_x, S_x) for the logits, through the same pass:
//   KL = A / S_t - lse_t + lse_x.
// Lanes merge by wave shuffles, waves through LDS; no atomics, so a row's value does not depend on the launch.  All sums
// are fp32; the last step of a row -- log(S), the quotient and the two differences -- is done once, by one lane, in fp64
// (a row's value is a difference of numbers of size lse ~ 10: rounding them to fp32 first would cost the result 1e-6).
//
// Special values follow torch: NaN anywhere in a row -> NaN (fmaxf drops a NaN from the maximum, but NaN - m reaches S);
// -inf logits are weight-0 terms; a label on a -inf logit -> +inf; a row of -inf only -> m = -inf, S = 0, -inf - -inf = NaN;
// +inf -> inf - inf = NaN.
#include <math.h>

#include <mutex>

#include "../gq_common.hpp"

namespace gq {
namespace {

constexpr int NT = 256;
constexpr int MAXK = 4096;
constexpr float L2E = 1.44269504088896340736f;

__device__ __forceinline__ float ex2(float v) { return __builtin_amdgcn_exp2f(v); }
// the reference point of the exponents: 0 while nothing finite has been seen (-inf - -inf would poison a row of -inf early)
__device__ __forceinline__ float ref_of(float m) { return m == -INFINITY ? 0.f : m; }

template <int DT> struct Ld;
template <> struct Ld<GQ_F32> {
    using E = float;
    static constexpr int VEC = 4;
    static __device__ __forceinline__ float one(const E* p) { return *p; }
    static __device__ __forceinline__ void vec(const uint4& w, float* x) {
        x[0] = __builtin_bit_cast(float, w.x), x[1] = __builtin_bit_cast(float, w.y);
        x[2] = __builtin_bit_cast(float, w.z), x[3] = __builtin_bit_cast(float, w.w);
    }
};
template <> struct Ld<GQ_F16> {
    using E = uint16_t;
    static constexpr int VEC = 8;
    static __device__ __forceinline__ float one(const E* p) { return h2f(*p); }
    static __device__ __forceinline__ void vec(const uint4& w, float* x) {
        const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) x[2 * i] = h2f((uint16_t)(u[i] & 0xffffu)), x[2 * i + 1] = h2f((uint16_t)(u[i] >> 16));
    }
};
template <> struct Ld<GQ_BF16> {
    using E = uint16_t;
    static constexpr int VEC = 8;
    static __device__ __forceinline__ float one(const E* p) { return bf2f(*p); }
    static __device__ __forceinline__ void vec(const uint4& w, float* x) {
        const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            x[2 * i] = __builtin_bit_cast(float, u[i] << 16), x[2 * i + 1] = __builtin_bit_cast(float, u[i] & 0xffff0000u);
    }
};

// head / body / tail of a row of V elements at p: [0, head) single elements, nvec 16-byte vectors, [tail0, V) single elements
template <typename E, int VEC>
struct Split {
    int head, ntail;
    int64_t nvec, tail0;
    __device__ __forceinline__ Split(const E* p, int64_t V) {
        const int mis = (int)((reinterpret_cast<uintptr_t>(p) / sizeof(E)) % VEC);
        const int64_t h = mis ? VEC - mis : 0;
        head = (int)(h < V ? h : V);
        nvec = (V - head) / VEC;
        tail0 = head + nvec * VEC;
        ntail = (int)(V - tail0);
    }
};

// ---- (m, S) of a softmax ----
struct MS {
    float m, s;
};
template <int N>
__device__ __forceinline__ void ms_add(MS& a, const float* x) {
    float vmax = x[0];
#pragma unroll
    for (int j = 1; j < N; ++j) vmax = fmaxf(vmax, x[j]);
    if (vmax > a.m) {  // (false for a NaN maximum: the NaN goes into S below)
        a.s *= ex2((a.m - vmax) * L2E);
        a.m = vmax;
    }
    const float r = ref_of(a.m);
#pragma unroll
    for (int j = 0; j < N; ++j) a.s += ex2((x[j] - r) * L2E);
}
__device__ __forceinline__ MS ms_merge(const MS& a, const MS& b) {
    const float M = fmaxf(a.m, b.m), r = ref_of(M);
    return {M, a.s * ex2((a.m - r) * L2E) + b.s * ex2((b.m - r) * L2E)};
}

// ---- the five running values of a KL row ----
struct KL5 {
    float mt, st, a, mx, sx;
};
template <int N>
__device__ __forceinline__ void kl_add(KL5& k, const float* t, const float* x) {
    float vmax = t[0];
#pragma unroll
    for (int j = 1; j < N; ++j) vmax = fmaxf(vmax, t[j]);
    if (vmax > k.mt) {
        const float f = ex2((k.mt - vmax) * L2E);
        k.st *= f, k.a *= f;
        k.mt = vmax;
    }
    const float r = ref_of(k.mt);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const float e = ex2((t[j] - r) * L2E);
        k.st += e;
        k.a += e * (t[j] - x[j]);
    }
    MS q{k.mx, k.sx};
    ms_add<N>(q, x);
    k.mx = q.m, k.sx = q.s;
}
__device__ __forceinline__ KL5 kl_merge(const KL5& a, const KL5& b) {
    const float M = fmaxf(a.mt, b.mt), r = ref_of(M);
    const float fa = ex2((a.mt - r) * L2E), fb = ex2((b.mt - r) * L2E);
    const MS q = ms_merge({a.mx, a.sx}, {b.mx, b.sx});
    return {M, a.st * fa + b.st * fb, a.a * fa + b.a * fb, q.m, q.s};
}

__device__ __forceinline__ MS shfl_xor(const MS& v, int d) { return {__shfl_xor(v.m, d), __shfl_xor(v.s, d)}; }
__device__ __forceinline__ KL5 shfl_xor(const KL5& v, int d) {
    return {__shfl_xor(v.mt, d), __shfl_xor(v.st, d), __shfl_xor(v.a, d), __shfl_xor(v.mx, d), __shfl_xor(v.sx, d)};
}
__device__ __forceinline__ MS merge(const MS& a, const MS& b) { return ms_merge(a, b); }
__device__ __forceinline__ KL5 merge(const KL5& a, const KL5& b) { return kl_merge(a, b); }

// every lane's value -> the workgroup's, valid in thread 0 (fixed order: xor butterfly inside a wave, then waves 0..3)
template <typename S>
__device__ __forceinline__ S block_merge(S v, S* lds) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = merge(v, shfl_xor(v, d));
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) lds[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) v = merge(v, lds[w]);
    }
    return v;
}

__device__ __forceinline__ double lse_of(float m, float s) { return (double)m + log((double)s); }

template <int DT>
__device__ __forceinline__ MS row_ms(const typename Ld<DT>::E* p, int64_t V) {
    using L = Ld<DT>;
    const int tid = threadIdx.x;
    const Split<typename L::E, L::VEC> sp(p, V);
    MS a{-INFINITY, 0.f};
    if (tid < sp.head) {
        const float x = L::one(p + tid);
        ms_add<1>(a, &x);
    }
    if (tid < sp.ntail) {
        const float x = L::one(p + sp.tail0 + tid);
        ms_add<1>(a, &x);
    }
    const uint4* body = reinterpret_cast<const uint4*>(p + sp.head);
#pragma unroll 2
    for (int64_t v = tid; v < sp.nvec; v += NT) {
        float x[L::VEC];
        L::vec(body[v], x);
        ms_add<L::VEC>(a, x);
    }
    return a;
}

template <int DT>
__global__ __launch_bounds__(NT) void nll_kernel(const typename Ld<DT>::E* __restrict__ logits, int64_t V, int64_t ld,
                                                 const int64_t* __restrict__ labels, int64_t ignore_index,
                                                 float* __restrict__ nll, float* __restrict__ lse, int* bad_label) {
    __shared__ MS lds[NT / 64];
    const int64_t t = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t label = labels[t];
    const bool ignored = label == ignore_index;
    if (!ignored && (label < 0 || label >= V)) {  // reported by the host as GQ_E_BAD_SHAPE; never read
        if (tid == 0) {
            nll[t] = NAN;
            if (lse) lse[t] = NAN;
            *bad_label = 1;
        }
        return;
    }
    if (ignored && !lse) {
        if (tid == 0) nll[t] = 0.f;
        return;
    }
    const typename Ld<DT>::E* p = logits + t * ld;
    const MS r = block_merge(row_ms<DT>(p, V), lds);
    if (tid == 0) {
        const double l = lse_of(r.m, r.s);
        if (lse) lse[t] = (float)l;
        nll[t] = ignored ? 0.f : (float)(l - (double)Ld<DT>::one(p + label));
    }
}

__device__ __forceinline__ float kl_value(const KL5& r) {
    return (float)((double)r.a / (double)r.st - lse_of(r.mt, r.st) + lse_of(r.mx, r.sx));
}

// VECP: logits and target have one element type and the same offset from a 16-byte boundary in every row
template <int DTX, int DTT, bool VECP>
__global__ __launch_bounds__(NT) void kl_kernel(const typename Ld<DTX>::E* __restrict__ logits,
                                                const typename Ld<DTT>::E* __restrict__ target, int64_t V, int64_t ld,
                                                int64_t ld_target, float* __restrict__ kl) {
    using LX = Ld<DTX>;
    using LT = Ld<DTT>;
    __shared__ KL5 lds[NT / 64];
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const typename LX::E* px = logits + row * ld;
    const typename LT::E* pt = target + row * ld_target;
    KL5 k{-INFINITY, 0.f, 0.f, -INFINITY, 0.f};
    if constexpr (VECP) {
        const Split<typename LX::E, LX::VEC> sp(px, V);
        if (tid < sp.head) {
            const float x = LX::one(px + tid), t = LT::one(pt + tid);
            kl_add<1>(k, &t, &x);
        }
        if (tid < sp.ntail) {
            const float x = LX::one(px + sp.tail0 + tid), t = LT::one(pt + sp.tail0 + tid);
            kl_add<1>(k, &t, &x);
        }
        const uint4* bx = reinterpret_cast<const uint4*>(px + sp.head);
        const uint4* bt = reinterpret_cast<const uint4*>(pt + sp.head);
#pragma unroll 2
        for (int64_t v = tid; v < sp.nvec; v += NT) {
            float x[LX::VEC], t[LX::VEC];
            LX::vec(bx[v], x);
            LT::vec(bt[v], t);
            kl_add<LX::VEC>(k, t, x);
        }
    } else {
        for (int64_t i = tid; i < V; i += NT) {
            const float x = LX::one(px + i), t = LT::one(pt + i);
            kl_add<1>(k, &t, &x);
        }
    }
    const KL5 r = block_merge(k, lds);
    if (tid == 0) kl[row] = kl_value(r);
}

template <int DTX, int DTT>
__global__ __launch_bounds__(NT) void kl_sparse_kernel(const typename Ld<DTX>::E* __restrict__ logits, int64_t V, int64_t ld,
                                                       const typename Ld<DTT>::E* __restrict__ tvals,
                                                       const int64_t* __restrict__ ids, int K, float* __restrict__ kl) {
    __shared__ KL5 lds[NT / 64];
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const typename Ld<DTX>::E* px = logits + row * ld;
    const typename Ld<DTT>::E* pt = tvals + row * K;
    const int64_t* pi = ids + row * K;
    KL5 k{-INFINITY, 0.f, 0.f, -INFINITY, 0.f};
    for (int i = tid; i < K; i += NT) {
        const int64_t id = pi[i];
        // an id outside [0, V) is not read: it makes the row NaN
        const float x = (id >= 0 && id < V) ? Ld<DTX>::one(px + id) : NAN, t = Ld<DTT>::one(pt + i);
        kl_add<1>(k, &t, &x);
    }
    const KL5 r = block_merge(k, lds);
    if (tid == 0) kl[row] = kl_value(r);
}

bool dtype_ok(int dt) { return dt == GQ_F32 || dt == GQ_F16 || dt == GQ_BF16; }
size_t esize(int dt) { return dt == GQ_F32 ? 4 : 2; }
bool elem_aligned(const void* p, int dt) { return (reinterpret_cast<uintptr_t>(p) & (esize(dt) - 1)) == 0; }

// the word the NLL kernel raises for a label outside [0, V): pinned host memory the device writes, one per process
std::mutex g_flag_mu;
int* g_flag_host = nullptr;

template <int DTX>
void launch_kl(const void* logits, const void* target, int tdt, bool vecp, int64_t T, int64_t V, int64_t ld, int64_t ldt, float* kl,
               hipStream_t st) {
    using EX = typename Ld<DTX>::E;
    const dim3 grid((unsigned)T), block(NT);
    if (vecp) {
        hipLaunchKernelGGL((kl_kernel<DTX, DTX, true>), grid, block, 0, st, (const EX*)logits, (const EX*)target, V, ld, ldt, kl);
        return;
    }
    switch (tdt) {
    case GQ_F32:
        hipLaunchKernelGGL((kl_kernel<DTX, GQ_F32, false>), grid, block, 0, st, (const EX*)logits, (const float*)target, V, ld, ldt, kl);
        break;
    case GQ_F16:
        hipLaunchKernelGGL((kl_kernel<DTX, GQ_F16, false>), grid, block, 0, st, (const EX*)logits, (const uint16_t*)target, V, ld, ldt, kl);
        break;
    default:
        hipLaunchKernelGGL((kl_kernel<DTX, GQ_BF16, false>), grid, block, 0, st, (const EX*)logits, (const uint16_t*)target, V, ld, ldt, kl);
        break;
    }
}

template <int DTX>
void launch_kl_sparse(const void* logits, const void* tvals, int tdt, const int64_t* ids, int64_t T, int64_t V, int64_t ld, int K,
                      float* kl, hipStream_t st) {
    using EX = typename Ld<DTX>::E;
    const dim3 grid((unsigned)T), block(NT);
    switch (tdt) {
    case GQ_F32:
        hipLaunchKernelGGL((kl_sparse_kernel<DTX, GQ_F32>), grid, block, 0, st, (const EX*)logits, V, ld, (const float*)tvals, ids, K, kl);
        break;
    case GQ_F16:
        hipLaunchKernelGGL((kl_sparse_kernel<DTX, GQ_F16>), grid, block, 0, st, (const EX*)logits, V, ld, (const uint16_t*)tvals, ids, K, kl);
        break;
    default:
        hipLaunchKernelGGL((kl_sparse_kernel<DTX, GQ_BF16>), grid, block, 0, st, (const EX*)logits, V, ld, (const uint16_t*)tvals, ids, K, kl);
        break;
    }
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_eval_nll(const void* logits, int dtype, int64_t T, int64_t V, int64_t ld, const int64_t* labels, int64_t ignore_index,
                float* nll, float* lse, void* stream) {
    if (int rc = options_ok()) return rc;
    if (!logits) GQ_FAIL(GQ_E_NULL, "gq_eval_nll: logits is NULL");
    if (!labels) GQ_FAIL(GQ_E_NULL, "gq_eval_nll: labels is NULL");
    if (!nll) GQ_FAIL(GQ_E_NULL, "gq_eval_nll: nll is NULL");
    if (!dtype_ok(dtype)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_eval_nll: unknown dtype %d", dtype);
    if (V <= 0) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_eval_nll: V=%ld must be positive", (long)V);
    if (T < 0 || T > 0x7fffffffLL) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_eval_nll: T=%ld outside [0, 2^31)", (long)T);
    if (ld < V) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_eval_nll: ld=%ld is smaller than V=%ld", (long)ld, (long)V);
    if (!elem_aligned(logits, dtype)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_eval_nll: logits is not aligned to its element size");
    if (T == 0) return GQ_OK;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(g_flag_mu);
    if (!g_flag_host) GQ_HIP(hipHostMalloc((void**)&g_flag_host, 64, hipHostMallocMapped | hipHostMallocPortable));
    int* flag_dev = nullptr;
    GQ_HIP(hipHostGetDevicePointer((void**)&flag_dev, g_flag_host, 0));
    *g_flag_host = 0;
    const dim3 grid((unsigned)T), block(NT);
    switch (dtype) {
    case GQ_F32:
        hipLaunchKernelGGL((nll_kernel<GQ_F32>), grid, block, 0, st, (const float*)logits, V, ld, labels, ignore_index, nll, lse, flag_dev);
        break;
    case GQ_F16:
        hipLaunchKernelGGL((nll_kernel<GQ_F16>), grid, block, 0, st, (const uint16_t*)logits, V, ld, labels, ignore_index, nll, lse, flag_dev);
        break;
    default:
        hipLaunchKernelGGL((nll_kernel<GQ_BF16>), grid, block, 0, st, (const uint16_t*)logits, V, ld, labels, ignore_index, nll, lse, flag_dev);
        break;
    }
    GQ_LAUNCH_CHECK();
    GQ_HIP(hipStreamSynchronize(st));  // the one entry point of this file that waits: its status depends on the labels
    if (*(volatile int*)g_flag_host)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_eval_nll: a label lies outside [0, V=%ld) and is not ignore_index=%ld (its row was not read; nll is NaN there)",
                (long)V, (long)ignore_index);
    return GQ_OK;
}

int gq_eval_kl(const void* logits, int dtype, const void* target, int target_dtype, int64_t T, int64_t V, int64_t ld,
               int64_t ld_target, float* kl, void* stream) {
    if (int rc = options_ok()) return rc;
    if (!logits) GQ_FAIL(GQ_E_NULL, "gq_eval_kl: logits is NULL");
    if (!target) GQ_FAIL(GQ_E_NULL, "gq_eval_kl: target is NULL");
    if (!kl) GQ_FAIL(GQ_E_NULL, "gq_eval_kl: kl is NULL");
    if (!dtype_ok(dtype)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_eval_kl: unknown dtype %d", dtype);
    if (!dtype_ok(target_dtype)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_eval_kl: unknown target_dtype %d", target_dtype);
    if (V <= 0) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_eval_kl: V=%ld must be positive", (long)V);
    if (T < 0 || T > 0x7fffffffLL) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_eval_kl: T=%ld outside [0, 2^31)", (long)T);
    if (ld < V) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_eval_kl: ld=%ld is smaller than V=%ld", (long)ld, (long)V);
    if (ld_target < V) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_eval_kl: ld_target=%ld is smaller than V=%ld", (long)ld_target, (long)V);
    if (!elem_aligned(logits, dtype) || !elem_aligned(target, target_dtype))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_eval_kl: logits / target not aligned to their element size");
    if (T == 0) return GQ_OK;
    // 16-byte loads of both operands need every row pair to sit at the same offset from a 16-byte boundary
    const size_t es = esize(dtype);
    const bool vecp = dtype == target_dtype &&
                      ((reinterpret_cast<uintptr_t>(logits) ^ reinterpret_cast<uintptr_t>(target)) & 15) == 0 &&
                      (T == 1 || (((uint64_t)ld * es) & 15) == (((uint64_t)ld_target * es) & 15));
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
    case GQ_F32: launch_kl<GQ_F32>(logits, target, target_dtype, vecp, T, V, ld, ld_target, kl, st); break;
    case GQ_F16: launch_kl<GQ_F16>(logits, target, target_dtype, vecp, T, V, ld, ld_target, kl, st); break;
    default: launch_kl<GQ_BF16>(logits, target, target_dtype, vecp, T, V, ld, ld_target, kl, st); break;
    }
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

int gq_eval_kl_sparse(const void* logits, int dtype, int64_t T, int64_t V, int64_t ld, const void* target_vals, int target_dtype,
                      const int64_t* target_ids, int64_t K, float* kl, void* stream) {
    if (int rc = options_ok()) return rc;
    if (!logits) GQ_FAIL(GQ_E_NULL, "gq_eval_kl_sparse: logits is NULL");
    if (!target_vals) GQ_FAIL(GQ_E_NULL, "gq_eval_kl_sparse: target_vals is NULL");
    if (!target_ids) GQ_FAIL(GQ_E_NULL, "gq_eval_kl_sparse: target_ids is NULL");
    if (!kl) GQ_FAIL(GQ_E_NULL, "gq_eval_kl_sparse: kl is NULL");
    if (!dtype_ok(dtype)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_eval_kl_sparse: unknown dtype %d", dtype);
    if (!dtype_ok(target_dtype)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_eval_kl_sparse: unknown target_dtype %d", target_dtype);
    if (V <= 0) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_eval_kl_sparse: V=%ld must be positive", (long)V);
    if (K <= 0 || K > MAXK) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_eval_kl_sparse: K=%ld outside [1, %d]", (long)K, MAXK);
    if (T < 0 || T > 0x7fffffffLL) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_eval_kl_sparse: T=%ld outside [0, 2^31)", (long)T);
    if (ld < V) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_eval_kl_sparse: ld=%ld is smaller than V=%ld", (long)ld, (long)V);
    if (!elem_aligned(logits, dtype) || !elem_aligned(target_vals, target_dtype) || (reinterpret_cast<uintptr_t>(target_ids) & 7))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_eval_kl_sparse: logits / target_vals / target_ids not aligned to their element size");
    if (T == 0) return GQ_OK;
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
    case GQ_F32: launch_kl_sparse<GQ_F32>(logits, target_vals, target_dtype, target_ids, T, V, ld, (int)K, kl, st); break;
    case GQ_F16: launch_kl_sparse<GQ_F16>(logits, target_vals, target_dtype, target_ids, T, V, ld, (int)K, kl, st); break;
    default: launch_kl_sparse<GQ_BF16>(logits, target_vals, target_dtype, target_ids, T, V, ld, (int)K, kl, st); break;
    }
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
