// gq_sample.hip -- K23: logits [B, V] -> one token id per row (include/gptq_gguf_sample.h): temperature, top-k, top-p and the
// inverse-CDF draw with the caller's random number, in ONE launch.  The torch expression of the same rule is a top-k (a sort),
// a softmax, a cumsum, a masked renormalisation and a multinomial with a host synchronise, per decode step.
//
// One workgroup of 1024 threads (16 waves) owns a row.  The row does not fit LDS at V = 128256; it is read from the caches
// once per pass.  Wave w takes a contiguous run of the row's 16-byte groups and lane l group l, l + 64, ... of that run, so the
// order (wave, turn, lane, element) IS the index order -- the tie rule below needs that.  Whole groups are one 16-byte load;
// the (at most two) groups that hang over the row's ends are read element by element, nothing outside [row, row + V).
//
//   pass 0  maximum with its lowest index, NaN flag.  NaN or a non-finite maximum: -1.  temperature == 0 or K == 1: done.
//   pass 1-4  exact radix select of the K-th largest key, 8 bits per pass, on an order-preserving uint32 image of the fp32
//           bits (-0 folded into +0).  Passes 1-3 count into a histogram that is replicated per LANE ([256 bins][64 lanes],
//           64 KB): the leading digits of logits fall into a handful of bins, and 64 lanes adding to one LDS word serialise.
//           With a copy per lane an instruction never meets itself; waves meet on a word only by chance.  Pass 4 counts per
//           WAVE ([16][256]): few keys are left, and the count of the threshold key in each wave is what the tie rule needs.
//           Integer adds: the counts do not depend on arrival order.
//   pass 5  compaction into LDS as (key << 32 | ~index): keys above the threshold in arrival order (the sort that follows
//           makes the order irrelevant), keys EQUAL to it by an ordered scan -- wave offsets from pass 4, lane offsets by a
//           shuffle scan -- so that exactly the lowest indices fill the `need` places left.
//   then    bitonic sort of the <= 1024 composites, descending: (z descending, index ascending).  w = expf((z - z0) / t), a
//           block scan in a fixed order, the nucleus and the draw as minima over j found with integer LDS atomics.
#include <math.h>

#include "../../../include/gptq_gguf_sample.h"
#include "../gq_common.hpp"

namespace gq {
namespace {

constexpr int NT = 1024, NW = NT / 64, MAXK = GQ_SAMPLE_MAX_K;
static_assert(MAXK <= NT, "one candidate per thread");

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

// One pass over the row: f(x, i0, lo, hi) with x[j] = z of index i0 + j for lo <= j < hi.  Every lane of a wave makes the
// same number of calls (a lane past its wave's run calls with lo == hi), so f may use wave collectives.
template <int DT, class F>
__device__ __forceinline__ void scan_row(const typename Ld<DT>::E* __restrict__ row, int64_t V, F&& f) {
    using L = Ld<DT>;
    constexpr int VEC = L::VEC;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int a = (int)((reinterpret_cast<uintptr_t>(row) / sizeof(typename L::E)) % VEC);  // elements past a 16-byte boundary
    const int64_t G = (V + a + VEC - 1) / VEC, gw = (G + NW - 1) / NW;
    const int64_t g0 = w * gw, g1 = g0 + gw < G ? g0 + gw : G;
    for (int64_t gb = g0; gb < g1; gb += 64) {
        const int64_t g = gb + lane, i0 = g * VEC - a;
        float x[VEC] = {};
        int lo = 0, hi = 0;
        if (g < g1) {
            if (i0 >= 0 && i0 + VEC <= V) {
                L::vec(*reinterpret_cast<const uint4*>(row + i0), x);
                hi = VEC;
            } else {
                lo = i0 < 0 ? (int)-i0 : 0;
                hi = V - i0 < VEC ? (int)(V - i0) : VEC;
#pragma unroll
                for (int j = 0; j < VEC; ++j) x[j] = (j >= lo && j < hi) ? L::one(row + i0 + j) : 0.f;
            }
        }
        f(x, i0, lo, hi);
    }
}

// larger z <=> larger key; -0 is +0 (they are equal as numbers, the rank order must not tell them apart)
__device__ __forceinline__ uint32_t key_of(float z) {
    if (z == 0.f) z = 0.f;
    const uint32_t u = __builtin_bit_cast(uint32_t, z);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float z_of(uint32_t k) {
    return __builtin_bit_cast(float, (k >> 31) ? (k & 0x7fffffffu) : ~k);
}

// inclusive scan over the 1024 threads in thread order; sw: NW entries.  A fixed order of additions.
template <typename T>
__device__ __forceinline__ T block_scan(T v, T* sw) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d, 64);
        if (lane >= d) v = o + v;
    }
    __syncthreads();  // (sw may still be read from the previous scan)
    if (lane == 63) sw[w] = v;
    __syncthreads();
    T off = 0;
    for (int i = 0; i < w; ++i) off = off + sw[i];
    return w ? off + v : v;
}

struct Shared {
    uint32_t hist[256 * 64];  // passes 1-3: [bin][lane]; pass 4: [wave][bin] in its first 16 KB
    uint64_t cand[MAXK];
    uint32_t tot[256];
    uint32_t scan_u[NW];
    float scan_f[NW];
    float wm[NW];
    int wi[NW];
    int wnan[NW];
    uint32_t sel_bin, sel_k;
    uint32_t ngt;
    int n, jhit, jlast;
    float S, Sn;
};

// the bin of tot[] that holds the krem-th largest key (bins from 255 down) -> bin; krem becomes the rank inside that bin
__device__ __forceinline__ uint32_t pick_bin(Shared& s, uint32_t& krem) {
    const int t = threadIdx.x;
    const uint32_t mine = t < 256 ? s.tot[255 - t] : 0u;
    const uint32_t incl = block_scan<uint32_t>(mine, s.scan_u);
    if (t < 256 && incl - mine < krem && krem <= incl) {
        s.sel_bin = 255 - t;
        s.sel_k = krem - (incl - mine);
    }
    __syncthreads();
    krem = s.sel_k;
    return s.sel_bin;
}

template <int DT, int SHIFT>
__device__ __forceinline__ void digit_pass(Shared& s, const typename Ld<DT>::E* row, int64_t V, uint32_t prefix) {
    constexpr int VEC = Ld<DT>::VEC;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    constexpr int WORDS = SHIFT ? 256 * 64 : NW * 256;
    for (int i = t; i < WORDS; i += NT) s.hist[i] = 0;
    __syncthreads();
    scan_row<DT>(row, V, [&](const float* x, int64_t, int lo, int hi) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (j < lo || j >= hi) continue;
            const uint32_t k = key_of(x[j]);
            if constexpr (SHIFT < 24) {
                if ((k ^ prefix) >> (SHIFT + 8)) continue;
            }
            const uint32_t d = (k >> SHIFT) & 255u;
            atomicAdd(&s.hist[SHIFT ? (d << 6) | lane : (w << 8) | d], 1u);
        }
    });
    __syncthreads();
    if (t < 256) {
        uint32_t c = 0;
        if constexpr (SHIFT != 0) {
            for (int j = 0; j < 64; ++j) c += s.hist[(t << 6) | ((j + t) & 63)];  // (rotated: the lanes of a wave on 64 banks)
        } else {
            for (int j = 0; j < NW; ++j) c += s.hist[(j << 8) | t];
        }
        s.tot[t] = c;
    }
    __syncthreads();
}

template <int DT>
__global__ __launch_bounds__(NT) void sample_kernel(const typename Ld<DT>::E* __restrict__ logits, int64_t V, int64_t ld, int K,
                                                     float top_p, float temperature, const float* __restrict__ u,
                                                     int64_t* __restrict__ ids) {
    constexpr int VEC = Ld<DT>::VEC;
    __shared__ Shared s;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t b = blockIdx.x;
    const typename Ld<DT>::E* row = logits + b * ld;

    // ---- pass 0: maximum, its lowest index, NaN ----
    float m = -INFINITY;
    int mi = 0x7fffffff;
    bool nan = false;
    scan_row<DT>(row, V, [&](const float* x, int64_t i0, int lo, int hi) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (j < lo || j >= hi) continue;
            nan |= x[j] != x[j];
            if (x[j] > m) m = x[j], mi = (int)(i0 + j);  // (ascending indices within a thread: the first of equals stays)
        }
    });
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const float om = __shfl_xor(m, d, 64);
        const int oi = __shfl_xor(mi, d, 64);
        if (om > m || (om == m && oi < mi)) m = om, mi = oi;
    }
    const bool wave_nan = __ballot(nan) != 0;
    if (lane == 0) s.wm[w] = m, s.wi[w] = mi, s.wnan[w] = wave_nan;
    if (t == 0) s.ngt = 0, s.jhit = 0x7fffffff, s.jlast = 0;
    __syncthreads();
    bool any_nan = false;
    m = s.wm[0], mi = s.wi[0];
    for (int i = 0; i < NW; ++i) {
        any_nan |= s.wnan[i] != 0;
        if (s.wm[i] > m || (s.wm[i] == m && s.wi[i] < mi)) m = s.wm[i], mi = s.wi[i];
    }
    if (any_nan || !(fabsf(m) < INFINITY)) {  // (uniform over the workgroup)
        if (t == 0) ids[b] = -1;
        return;
    }
    if (temperature == 0.f || K == 1) {
        if (t == 0) ids[b] = mi;
        return;
    }

    // ---- passes 1-4: the K-th largest key ----
    uint32_t krem = (uint32_t)K, thr = 0;
    digit_pass<DT, 24>(s, row, V, thr);
    thr |= pick_bin(s, krem) << 24;
    digit_pass<DT, 16>(s, row, V, thr);
    thr |= pick_bin(s, krem) << 16;
    digit_pass<DT, 8>(s, row, V, thr);
    thr |= pick_bin(s, krem) << 8;
    digit_pass<DT, 0>(s, row, V, thr);
    const uint32_t bin0 = pick_bin(s, krem);
    thr |= bin0;
    const uint32_t need = krem, base = (uint32_t)K - need;  // `need` places for keys == thr, K - need keys are above it
    uint32_t tie_off = 0;                                   // keys == thr in the waves before this one
    for (int i = 0; i < w; ++i) tie_off += s.hist[(i << 8) | bin0];

    // ---- pass 5: the candidates ----
    int n2 = 2;
    while (n2 < K) n2 <<= 1;
    if (t >= K && t < n2) s.cand[t] = 0;  // (below every real composite: keys are >= 0x007fffff)
    scan_row<DT>(row, V, [&](const float* x, int64_t i0, int lo, int hi) {
        int c = 0;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (j < lo || j >= hi) continue;
            const uint32_t k = key_of(x[j]);
            if (k > thr) {
                const uint32_t slot = atomicAdd(&s.ngt, 1u);  // (< base by the select; the check keeps a bug inside cand)
                if (slot < base) s.cand[slot] = ((uint64_t)k << 32) | (uint32_t)~(uint32_t)(i0 + j);
            }
            c += k == thr;
        }
        if (tie_off >= need || __ballot(c != 0) == 0) return;  // (both wave-uniform)
        int incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        uint32_t r = tie_off + (uint32_t)(incl - c);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (j < lo || j >= hi || key_of(x[j]) != thr) continue;
            if (r < need) s.cand[base + r] = ((uint64_t)thr << 32) | (uint32_t)~(uint32_t)(i0 + j);
            ++r;
        }
        tie_off += (uint32_t)__shfl(incl, 63, 64);
    });

    // ---- (z descending, index ascending) ----
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            const int p = t ^ j;
            if (t < n2 && p > t) {
                const uint64_t ca = s.cand[t], cb = s.cand[p];
                if ((ca < cb) == ((t & k) == 0)) s.cand[t] = cb, s.cand[p] = ca;
            }
        }
    __syncthreads();

    // ---- weights, nucleus, draw ----
    const float z0 = z_of((uint32_t)(s.cand[0] >> 32));
    const float wj = t < K ? expf((z_of((uint32_t)(s.cand[t < K ? t : 0] >> 32)) - z0) / temperature) : 0.f;
    const float P = block_scan<float>(wj, s.scan_f);
    if (t == K - 1) s.S = P, s.n = K;
    __syncthreads();
    if (top_p != 1.f && t < K && P >= top_p * s.S) atomicMin(&s.n, t + 1);
    __syncthreads();
    const int n = s.n;
    if (t == n - 1) s.Sn = P;
    __syncthreads();
    if (t < n) {
        if (P > u[b] * s.Sn) atomicMin(&s.jhit, t);
        if (wj > 0.f) atomicMax(&s.jlast, t);
    }
    __syncthreads();
    if (t == 0) {
        const int j = s.jhit < n ? s.jhit : s.jlast;
        ids[b] = (int64_t)(~(uint32_t)s.cand[j] & 0x7fffffffu);
    }
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_sample_logits(const void* logits, int dtype, int64_t B, int64_t V, int64_t ld, int top_k, float top_p, float temperature,
                     const float* u, int64_t* ids, void* stream) {
    if (int rc = options_ok()) return rc;
    if (dtype != GQ_F32 && dtype != GQ_F16 && dtype != GQ_BF16)
        GQ_FAIL(GQ_E_BAD_TYPE, "gq_sample_logits: unknown dtype %d (GQ_F32, GQ_F16 or GQ_BF16)", dtype);
    if (!logits) GQ_FAIL(GQ_E_NULL, "gq_sample_logits: logits is NULL");
    if (!ids) GQ_FAIL(GQ_E_NULL, "gq_sample_logits: ids is NULL");
    if (B < 1 || B > 0x7fffffffLL) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_sample_logits: B=%ld (not in [1, 2^31))", (long)B);
    if (V < 1 || V > 0x7fffffffLL) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_sample_logits: V=%ld (not in [1, 2^31))", (long)V);
    if (ld < V) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_sample_logits: ld=%ld is smaller than V=%ld", (long)ld, (long)V);
    if (top_k < 1 || top_k > GQ_SAMPLE_MAX_K)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_sample_logits: top_k=%d (not in [1, %d]; an unbounded nucleus is not built)", top_k,
                GQ_SAMPLE_MAX_K);
    if (!(top_p > 0.f && top_p <= 1.f)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_sample_logits: top_p=%g (not in (0, 1])", (double)top_p);
    if (!(temperature >= 0.f))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_sample_logits: temperature=%g (negative or NaN; 0 is the argmax)", (double)temperature);
    if (!u && temperature > 0.f) GQ_FAIL(GQ_E_NULL, "gq_sample_logits: u is NULL with temperature=%g > 0", (double)temperature);
    if (!aligned(logits, dtype == GQ_F32 ? 4 : 2)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_sample_logits: logits is not aligned to its element size");
    if (!aligned(u, 4)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_sample_logits: u not 4-byte aligned");
    if (!aligned(ids, 8)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_sample_logits: ids not 8-byte aligned");
    const int K = (int)(top_k < V ? top_k : V);
    const dim3 grid((unsigned)B), block(NT);
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
    case GQ_F32:
        hipLaunchKernelGGL((sample_kernel<GQ_F32>), grid, block, 0, st, (const float*)logits, V, ld, K, top_p, temperature, u, ids);
        break;
    case GQ_F16:
        hipLaunchKernelGGL((sample_kernel<GQ_F16>), grid, block, 0, st, (const uint16_t*)logits, V, ld, K, top_p, temperature, u, ids);
        break;
    default:
        hipLaunchKernelGGL((sample_kernel<GQ_BF16>), grid, block, 0, st, (const uint16_t*)logits, V, ld, K, top_p, temperature, u, ids);
        break;
    }
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
