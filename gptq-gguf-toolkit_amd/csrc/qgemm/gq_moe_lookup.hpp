// gq_moe_lookup.hpp -- how a workgroup of a grouped expert GEMM finds its (expert, token tile) from gq_moe_route's
// expert_start: E + 1 <= 257 values, five per lane, the number of token tiles of a lane's four experts, one prefix sum over the
// wave and a ballot.  Every wave of the workgroup computes the same answer, so no LDS and no barrier is spent on it.
// gq_moe_gemm.hip (K25) and gq_moe_gemm_a8.hip (K36) include it; the grouped expert GEMVs (K24, K38) take nth_set_bit from
// here.  Device code only.
#pragma once
#include "../../../include/gptq_gguf_moe_gemm.h"
#include "../gq_common.hpp"

namespace gq {
namespace moelookup {

constexpr int MAXE = GQ_MOE_ROUTE_MAX_EXPERTS, PER = MAXE / 64;  // experts per lane of a wave-wide scan
static_assert(MAXE % 64 == 0, "four experts per lane");

// the position of the n-th (from 0) set bit of m, n < popcount(m): six halvings, no cross-lane traffic.  The grouped expert
// GEMVs (gq_moe_gemv.hip, K24; gq_moe_gemv_a8.hip, K38) find the pairs of their expert's ballot mask with it.
__device__ __forceinline__ int nth_set_bit(uint64_t m, int n) {
    int pos = 0;
#pragma unroll
    for (int w = 32; w; w >>= 1) {
        const int c = __builtin_popcountll((m >> pos) & ((1ull << w) - 1));
        if (n >= c) n -= c, pos += w;
    }
    return pos;
}

// inclusive prefix sum of v over the 64 lanes
__device__ __forceinline__ int wave_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// Token tile b of the grid, with TT tokens per tile: -> whether an expert holds it (uniform over the workgroup), and then the
// expert e, the first position pos0 of the tile inside `order` and the number cnt <= TT of its pairs.
template <int TT>
__device__ __forceinline__ bool expert_tile(const int32_t* __restrict__ expert_start, int E, int b, int lane, int& e, int& pos0,
                                            int& cnt) {
    // lane l holds the starts of experts 4 l .. 4 l + 3 and the end of the last
    int st[PER + 1], nt[PER], s = 0;
#pragma unroll
    for (int k = 0; k <= PER; ++k) {
        const int x = PER * lane + k;
        st[k] = expert_start[x < E ? x : E];
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) s += nt[k] = (st[k + 1] - st[k] + TT - 1) / TT;  // (0 from E on: equal starts)
    const int inc = wave_scan(s, lane);
    const uint64_t hit = __ballot(b >= inc - s && b < inc);
    if (hit == 0) return false;
    e = 0, pos0 = 0, cnt = 0;
    int bb = b - (inc - s);
    bool found = false;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (!found && bb < nt[k]) {
            found = true, e = PER * lane + k, pos0 = st[k] + bb * TT;
            cnt = st[k + 1] - pos0 < TT ? st[k + 1] - pos0 : TT;
        }
        bb -= nt[k];
    }
    const int src = __builtin_ctzll(hit);
    e = __shfl(e, src), pos0 = __shfl(pos0, src), cnt = __shfl(cnt, src);
    return true;
}

}  // namespace moelookup
}  // namespace gq
