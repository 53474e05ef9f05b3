// gq_moe_combine.hip -- K29: the last step of the calibration forward of a fused-expert MoE layer.  transformers'
// MixtralExperts.forward ends every hit expert with
//     h = h * top_k_weights[token_idx, top_k_pos, None];  final.index_add_(0, token_idx, h.to(final.dtype))
// -- 3 E launches over [n_e, H] slices.  gq_fwd_moe_combine does all of them in ONE launch over the expert-sorted [P, H] matrix
// of down-projection outputs, with the same roundings: per (token, element) the products are rounded to the 16-bit type and
// added, in ascending expert id, to an accumulator that is rounded to the 16-bit type after every add and starts at +0.
//
// A workgroup takes a token (the grid is capped, the tokens strided over it).  Lanes 0 .. K - 1 of wave 0 each look one of the
// token's pairs up: expert id, weight, and the row of y -- the position of pair p = k T + t in `order`, found by a binary
// search in its expert's run, which gq_moe_route leaves ascending (no inverse of `order`, no workspace).  The K entries are
// ranked by (expert, k) with shuffles -- a sort in registers -- and left in LDS in that order.  Then every lane streams: K
// 16-byte loads of y, one 16-byte store of out per 8 elements.  Memory-bound: (K + 1) * 2 H bytes per token.
#include "../../../include/gptq_gguf_moe_calib.h"

#include "../gq_common.hpp"

namespace gq {
namespace {

constexpr int MAXK = GQ_MOE_COMBINE_MAX_K;
constexpr int COMBINE_GRID_CAP = 2048;  // 256 CUs x 8 workgroups: the rest of the tokens are strided

template <bool BF16> __device__ __forceinline__ float ld16(uint16_t v) { return BF16 ? bf2f(v) : h2f(v); }
template <bool BF16> __device__ __forceinline__ uint16_t st16(float f) { return BF16 ? f2bf(f) : f2h(f); }

template <bool BF16, bool W32>
__global__ __launch_bounds__(256) void fwd_moe_combine_kernel(const uint16_t* __restrict__ y, const int32_t* __restrict__ pair_expert,
                                                              const int32_t* __restrict__ expert_start,
                                                              const int32_t* __restrict__ order, const void* __restrict__ w, int T,
                                                              int K, int E, int H8, uint16_t* __restrict__ out) {
    __shared__ int32_t srow[MAXK];  // rows of y of the token's valid pairs, in the order they are added
    __shared__ float sw[MAXK];      // their weights
    __shared__ int32_t sn;          // how many
    const int tid = threadIdx.x, P = T * K;
    const int64_t H = (int64_t)H8 * 8;
    for (int t = blockIdx.x; t < T; t += gridDim.x) {
        if (tid < 64) {
            int e = -1, s = -1;
            float wk = 0.0f;
            if (tid < K) {
                const int p = tid * T + t;
                e = pair_expert[p];
                if ((unsigned)e < (unsigned)E) {
                    int lo = expert_start[e], hi = expert_start[e + 1];
                    lo = lo < 0 ? 0 : lo, hi = hi > P ? P : hi;
                    while (lo < hi) {  // the first position of the run that holds a pair >= p
                        const int mid = (lo + hi) >> 1;
                        if (order[mid] < p) lo = mid + 1;
                        else hi = mid;
                    }
                    const int end = expert_start[e + 1] > P ? P : expert_start[e + 1];
                    if (lo < end && order[lo] == p) s = lo;
                    wk = W32 ? static_cast<const float*>(w)[t * K + tid] : ld16<BF16>(static_cast<const uint16_t*>(w)[t * K + tid]);
                }
            }
            const bool valid = s >= 0;
            int rank = 0;  // the valid entries with a smaller (expert, k)
#pragma unroll
            for (int j = 0; j < MAXK; ++j) {
                const int ej = __shfl(e, j), sj = __shfl(s, j);
                if (sj >= 0 && (ej < e || (ej == e && j < tid))) ++rank;
            }
            if (valid) srow[rank] = s, sw[rank] = wk;
            const uint64_t m = __ballot(valid);
            if (tid == 0) sn = __builtin_popcountll(m);
        }
        __syncthreads();
        const int n = sn;
        for (int c = tid; c < H8; c += blockDim.x) {
            uint4 v[MAXK];
#pragma unroll
            for (int i = 0; i < MAXK; ++i)
                if (i < n) v[i] = *reinterpret_cast<const uint4*>(y + (int64_t)srow[i] * H + 8 * c);
            float acc[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
#pragma unroll
            for (int i = 0; i < MAXK; ++i) {
                if (i < n) {
                    const float wi = sw[i];
                    const uint32_t V[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float prod = ld16<BF16>(st16<BF16>(ld16<BF16>((uint16_t)(V[j >> 1] >> (16 * (j & 1)))) * wi));
                        acc[j] = ld16<BF16>(st16<BF16>(acc[j] + prod));  // (+0) + (-0) = +0: the first product is added too
                    }
                }
            }
            uint32_t o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                o[j] = (uint32_t)st16<BF16>(acc[2 * j]) | ((uint32_t)st16<BF16>(acc[2 * j + 1]) << 16);
            *reinterpret_cast<uint4*>(out + (int64_t)t * H + 8 * c) = make_uint4(o[0], o[1], o[2], o[3]);
        }
        __syncthreads();  // the next token's entries overwrite srow / sw / sn
    }
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_fwd_moe_combine(const void* y, const int32_t* pair_expert, const int32_t* expert_start, const int32_t* order,
                       const void* w, int w_dtype, int64_t T, int64_t K, int64_t E, int64_t H, int dtype, void* out,
                       void* stream) {
    if (int rc = options_ok()) return rc;
    if (dtype != GQ_F16 && dtype != GQ_BF16) GQ_FAIL(GQ_E_BAD_TYPE, "gq_fwd_moe_combine: dtype %d (fp16 / bf16)", dtype);
    if (w_dtype != GQ_F32 && w_dtype != dtype)
        GQ_FAIL(GQ_E_BAD_TYPE, "gq_fwd_moe_combine: w_dtype %d (fp32, or the dtype %d of y)", w_dtype, dtype);
    if (!y) GQ_FAIL(GQ_E_NULL, "gq_fwd_moe_combine: y is NULL");
    if (!pair_expert) GQ_FAIL(GQ_E_NULL, "gq_fwd_moe_combine: pair_expert is NULL");
    if (!expert_start) GQ_FAIL(GQ_E_NULL, "gq_fwd_moe_combine: expert_start is NULL");
    if (!order) GQ_FAIL(GQ_E_NULL, "gq_fwd_moe_combine: order is NULL");
    if (!w) GQ_FAIL(GQ_E_NULL, "gq_fwd_moe_combine: w is NULL");
    if (!out) GQ_FAIL(GQ_E_NULL, "gq_fwd_moe_combine: out is NULL");
    if (E < 1 || E > GQ_MOE_ROUTE_MAX_EXPERTS)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_fwd_moe_combine: E=%ld (not in [1, %d] experts)", (long)E, GQ_MOE_ROUTE_MAX_EXPERTS);
    if (K < 1 || K > GQ_MOE_COMBINE_MAX_K)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_fwd_moe_combine: K=%ld (not in [1, %d] experts per token)", (long)K, GQ_MOE_COMBINE_MAX_K);
    if (T < 1 || T > GQ_MOE_ROUTE_MAX_PAIRS / K)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_fwd_moe_combine: T=%ld (T * K not in [1, %d] pairs, K=%ld)", (long)T, GQ_MOE_ROUTE_MAX_PAIRS, (long)K);
    if (H < 8 || H % 8 || H > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_fwd_moe_combine: H=%ld (H %% 8, H >= 8)", (long)H);
    if (!aligned(y, 16)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_fwd_moe_combine: y not 16-byte aligned");
    if (!aligned(out, 16)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_fwd_moe_combine: out not 16-byte aligned");
    if (!aligned(pair_expert, 4)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_fwd_moe_combine: pair_expert not 4-byte aligned");
    if (!aligned(expert_start, 4)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_fwd_moe_combine: expert_start not 4-byte aligned");
    if (!aligned(order, 4)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_fwd_moe_combine: order not 4-byte aligned");
    if (!aligned(w, w_dtype == GQ_F32 ? 4 : 2))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_fwd_moe_combine: w not %d-byte aligned", w_dtype == GQ_F32 ? 4 : 2);
    const int H8 = (int)(H / 8);
    const dim3 grid((unsigned)(T < COMBINE_GRID_CAP ? T : COMBINE_GRID_CAP)), block(H8 <= 64 ? 64 : H8 <= 128 ? 128 : 256);
    hipStream_t st = (hipStream_t)stream;
#define GQ_COMBINE(B16, W32)                                                                                                  \
    hipLaunchKernelGGL((fwd_moe_combine_kernel<B16, W32>), grid, block, 0, st, static_cast<const uint16_t*>(y), pair_expert, \
                       expert_start, order, w, (int)T, (int)K, (int)E, H8, static_cast<uint16_t*>(out))
    const bool w32 = w_dtype == GQ_F32;
    if (dtype == GQ_BF16) { if (w32) GQ_COMBINE(true, true); else GQ_COMBINE(true, false); }
    else { if (w32) GQ_COMBINE(false, true); else GQ_COMBINE(false, false); }
#undef GQ_COMBINE
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
