// gq_moe_gemm.hip -- K25: the prefill of a packed MoE layer.  gq_moe_route sorts the router's (token, expert) pairs by expert
// on the device; gq_linear_packed_experts multiplies every pair with its expert's weight, read as the GGUF block bytes of the
// stacked [E, R, C] tensor, in one launch of K21's tile kernel.  The expert ids, the counts and the order stay on the device;
// nothing is read back.
//
// Route: ONE workgroup of 1024 threads (P <= 2^17 ids are 512 KB, read twice: not worth a second launch or a workspace).
//   1. counts per expert with LDS integer atomics (a sum of ones: the arrival order does not show), then an exclusive scan by
//      wave 0, four experts per lane -> expert_start.
//   2. positions, by an ordered scan: the pairs are taken in chunks of 1024 in pair order.  Inside a wave a lane's rank among
//      the earlier lanes with its expert comes from ballots (one per distinct expert of the wave), the wave's count per expert
//      goes to wc[wave][e]; a pair's position is base[e] + the counts of the lower waves + its rank, and base[e] then advances
//      by the chunk's total.  Three barriers per chunk, no atomic decides a position.
//   3. order[expert_start[E] .. P) = -1.
//
// GEMM: workgroup (row tile, token tile b) of the grid n_rt x (ceil(P / TT) + min(E, P)).  Every wave reads expert_start
// (E + 1 <= 257 values, five per lane), forms the number of token tiles of its four experts, prefix-sums them over the wave
// and finds the expert whose tiles hold b and the first position of the tile inside that expert's run -- the same in all four
// waves, so no LDS and no barrier is spent on it.  No expert holds b: the workgroup returns before any staging.  Tile token i
// is then pair order[pos0 + i]: its x row is (pair / pairs_per_row), its y row the pair.  The x row indices of a thread's XP
// loads stay in registers through the K loop; the y rows are read again from `order` (L2) in the epilogue.
// The K loop, the staging and the epilogue are gq_qgemm_core.hpp's tile_pass, the text gq_linear_packed runs.
#include "../../../include/gptq_gguf_moe_gemm.h"

#include "../search/gq_block_host.hpp"
#include "gq_qgemm_core.hpp"

namespace gq {
namespace {

using namespace gemmcore;

constexpr int MAXE = GQ_MOE_ROUTE_MAX_EXPERTS, PER = MAXE / 64;  // experts per lane of a wave-wide scan
constexpr int RT = 1024, RW = RT / 64;                           // threads and waves of the route workgroup
static_assert(MAXE % 64 == 0 && MAXE <= RT, "four experts per lane; one thread per expert");

// inclusive prefix sum of v over the 64 lanes
__device__ __forceinline__ int wave_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

__global__ __launch_bounds__(RT) void moe_route_kernel(const int32_t* __restrict__ pair_expert, int P, int E,
                                                       int32_t* __restrict__ expert_start, int32_t* __restrict__ order) {
    __shared__ int32_t base[MAXE + 1];  // counts, then starts, then the next free position of every expert
    __shared__ int32_t wc[RW * MAXE];   // [wave][e]: the wave's pairs of expert e in the current chunk
    __shared__ int32_t total;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i <= MAXE; i += RT) base[i] = 0;
    for (int i = tid; i < RW * MAXE; i += RT) wc[i] = 0;
    __syncthreads();
    for (int i = tid; i < P; i += RT) {
        const int e = pair_expert[i];
        if ((unsigned)e < (unsigned)E) atomicAdd(&base[e], 1);
    }
    __syncthreads();
    if (wave == 0) {
        int c[PER], s = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) s += c[k] = base[PER * lane + k];  // (zero from E on)
        int at = wave_scan(s, lane) - s;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int e = PER * lane + k;
            if (e < E) base[e] = at, expert_start[e] = at;
            at += c[k];
        }
        if (lane == 63) total = at, expert_start[E] = at;  // the number of valid pairs (E may be MAXE: no lane's expert)
    }
    __syncthreads();
    const int n_valid = total;
    const uint64_t below = (1ull << lane) - 1;
    for (int i0 = 0; i0 < P; i0 += RT) {
        const int i = i0 + tid, e = i < P ? pair_expert[i] : -1;
        const bool valid = (unsigned)e < (unsigned)E;
        int rank = 0;
        for (uint64_t todo = __ballot(valid); todo;) {  // one turn per distinct expert of the wave: uniform
            const int src = __builtin_ctzll(todo), e0 = __shfl(e, src);
            const uint64_t m = __ballot(valid && e == e0);
            if (valid && e == e0) rank = __builtin_popcountll(m & below);
            if (lane == src) wc[wave * MAXE + e0] = __builtin_popcountll(m);
            todo &= ~m;
        }
        __syncthreads();
        if (valid) {
            int pos = base[e] + rank;
            for (int w = 0; w < wave; ++w) pos += wc[w * MAXE + e];
            if (pos < P) order[pos] = i;  // (always, unless pair_expert changed between the two passes)
        }
        __syncthreads();
        if (tid < E) {  // the thread that reads a column also clears it for the next chunk
            int s = 0;
#pragma unroll
            for (int w = 0; w < RW; ++w) s += wc[w * MAXE + tid], wc[w * MAXE + tid] = 0;
            base[tid] += s;
        }
        __syncthreads();
    }
    for (int i = n_valid + tid; i < P; i += RT) order[i] = -1;
}

template <int QT, bool BF16, int TT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void linear_packed_experts_kernel(
    const uint8_t* __restrict__ blocks, int E, int64_t R, int64_t C, const uint8_t* __restrict__ x, int pairs_per_row,
    const int32_t* __restrict__ expert_start, const int32_t* __restrict__ order, int P, uint16_t* __restrict__ y, uint32_t n_rt) {
    using Q = QL<QT>;
    constexpr int XP = TT * 8 / 256;
    __shared__ __attribute__((aligned(16))) uint8_t sb[TR * Q::SLOT];
    __shared__ __attribute__((aligned(16))) uint8_t sx[TT * KC * 2];
    __shared__ int64_t sbase[TR];
    const int tid = threadIdx.x, lane = tid & 63;
    const int b = blockIdx.x / n_rt;  // row tiles fastest: they share x and the expert
    // this workgroup's (expert, tile): lane l holds the starts of experts 4 l .. 4 l + 3 and the end of the last
    int st[PER + 1], nt[PER], s = 0;
#pragma unroll
    for (int k = 0; k <= PER; ++k) {
        const int e = PER * lane + k;
        st[k] = expert_start[e < E ? e : E];
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) s += nt[k] = (st[k + 1] - st[k] + TT - 1) / TT;  // (0 from E on: equal starts)
    const int inc = wave_scan(s, lane);
    const uint64_t hit = __ballot(b >= inc - s && b < inc);
    if (hit == 0) return;  // uniform over the workgroup: every wave read the same starts
    int e = 0, pos0 = 0, cnt = 0;
    {
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
    }
    const int64_t r0 = (int64_t)(blockIdx.x % n_rt) * TR;
    const int nr = (int)((R - r0) < TR ? (R - r0) : TR), ntt = (cnt + 15) >> 4;
    const int64_t nsb = C / 256;
    if (tid < nr) sbase[tid] = ((int64_t)e * R + r0 + tid) * nsb * Q::ROWB;
    // the pair of tile token i, or -1: a position outside [0, P) and an entry outside [0, P) are never followed
    auto pair_of = [=](int i) {
        const int at = pos0 + i;
        const int p = i < cnt && (unsigned)at < (unsigned)P ? order[at] : -1;
        return (unsigned)p < (unsigned)P ? p : -1;
    };
    int xrow[XP];
#pragma unroll
    for (int i = 0; i < XP; ++i) {
        const int p = pair_of((tid + 256 * i) >> 3);
        xrow[i] = p < 0 ? -1 : p / pairs_per_row;
    }
    tile_pass<QT, BF16, TT>(
        blocks, sbase, nr, ntt, r0, R, C, x, [&](int i) { return Row{xrow[i] >= 0, (int64_t)xrow[i]}; }, y,
        [=](int tt) {
            const int p = pair_of(16 * tt + (tid & 15));
            return Row{p >= 0, (int64_t)p};
        },
        sb, sx);
}

// The 256-token tile of Q4_K / Q5_K / IQ4_XS does not fit 256 registers in this text (K21's own four Q4_K / Q5_K instances spill
// 160-208 bytes per lane and it builds none for IQ4_XS; with the gathered row indices it is 16 more): the grouped kernel does not
// have it, so that no instance of it uses scratch.
constexpr bool wide_ok(int q_type) { return q_type != GQ_Q4_K && q_type != GQ_Q5_K && q_type != GQ_IQ4_XS; }

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_moe_route(const int32_t* pair_expert, int64_t P, int64_t E, int32_t* expert_start, int32_t* order, void* stream) {
    if (int rc = options_ok()) return rc;
    if (!pair_expert) GQ_FAIL(GQ_E_NULL, "gq_moe_route: pair_expert is NULL");
    if (!expert_start) GQ_FAIL(GQ_E_NULL, "gq_moe_route: expert_start is NULL");
    if (!order) GQ_FAIL(GQ_E_NULL, "gq_moe_route: order is NULL");
    if (E < 1 || E > GQ_MOE_ROUTE_MAX_EXPERTS)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_moe_route: E=%ld (not in [1, %d] experts)", (long)E, GQ_MOE_ROUTE_MAX_EXPERTS);
    if (P < 1 || P > GQ_MOE_ROUTE_MAX_PAIRS)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_moe_route: P=%ld (not in [1, %d] pairs)", (long)P, GQ_MOE_ROUTE_MAX_PAIRS);
    if (!aligned(pair_expert, 4)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_moe_route: pair_expert not 4-byte aligned");
    if (!aligned(expert_start, 4)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_moe_route: expert_start not 4-byte aligned");
    if (!aligned(order, 4)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_moe_route: order not 4-byte aligned");
    hipLaunchKernelGGL(moe_route_kernel, dim3(1), dim3(RT), 0, (hipStream_t)stream, pair_expert, (int)P, (int)E, expert_start, order);
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

int gq_linear_packed_experts(int q_type, const void* blocks, int64_t E, int64_t R, int64_t C, const void* x, int64_t x_rows,
                             int64_t pairs_per_row, const int32_t* expert_start, const int32_t* order, int64_t P, int x_dtype,
                             void* y, void* stream) {
    if (int rc = options_ok()) return rc;
    const char* who = "gq_linear_packed_experts";
    if (int rc = check_types(who, q_type, x_dtype)) return rc;
    if (int rc = need(who, "blocks", blocks)) return rc;
    if (int rc = need(who, "x", x)) return rc;
    if (int rc = need(who, "expert_start", expert_start)) return rc;
    if (int rc = need(who, "order", order)) return rc;
    if (int rc = need(who, "y", y)) return rc;
    if (E < 1 || E > GQ_MOE_ROUTE_MAX_EXPERTS)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_linear_packed_experts: E=%ld (not in [1, %d] experts)", (long)E, GQ_MOE_ROUTE_MAX_EXPERTS);
    if (int rc = check_R(who, R)) return rc;
    if (P < 1 || P > GQ_MOE_ROUTE_MAX_PAIRS)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_linear_packed_experts: P=%ld (not in [1, %d] pairs)", (long)P, GQ_MOE_ROUTE_MAX_PAIRS);
    if (int rc = check_pairs(who, x_rows, pairs_per_row, P)) return rc;
    if (int rc = check_C256(who, C)) return rc;
    if (int rc = check_blocks_aligned(who, q_type, blocks)) return rc;
    if (int rc = check_aligned(who, "expert_start", expert_start, 4)) return rc;
    if (int rc = check_aligned(who, "order", order, 4)) return rc;
    if (int rc = check_aligned(who, "x", x, 16)) return rc;
    if (int rc = check_aligned(who, "y", y, 16)) return rc;
    // The host does not know the counts, it knows their mean: the 256-token tile is taken when a run is on average at least one
    // 128-token tile long.  About half of the runs or more then overflow a 128-token tile, which decodes the expert's rows once
    // more for the rest, while a 256-token tile that is half empty skips the matrix instructions of its empty half (K25 has both
    // widths measured).
    const int64_t n_rt = (R + TR - 1) / TR;
    const bool wide = wide_ok(q_type) && P >= 128 * E;
    const int tt = wide ? 256 : 128;
    const int64_t n_tt = (P + tt - 1) / tt + (E < P ? E : P);  // <= 2^10 + 2^8
    if (n_rt > 0x7fffffff / n_tt)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_linear_packed_experts: R=%ld P=%ld is more than one launch takes", (long)R, (long)P);
    const dim3 grid((unsigned)(n_rt * n_tt));
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* b = static_cast<const uint8_t*>(blocks);
    const uint8_t* xp = static_cast<const uint8_t*>(x);
    uint16_t* yp = static_cast<uint16_t*>(y);
    dispatch_packed(q_type, [&](auto qt) {
        constexpr int QT = decltype(qt)::value;
        dispatch_bool(x_dtype == GQ_BF16, [&](auto bf16) {
            auto go = [&](auto w) {  // w: the 256-token tile
                hipLaunchKernelGGL((linear_packed_experts_kernel<QT, decltype(bf16)::value, decltype(w)::value ? 256 : 128>), grid,
                                   dim3(256), 0, st, b, (int)E, R, C, xp, (int)pairs_per_row, expert_start, order, (int)P, yp,
                                   (uint32_t)n_rt);
            };
            if constexpr (wide_ok(QT)) dispatch_bool(wide, go);  // (no 256-token instance is built for the other types)
            else go(std::false_type{});
        });
    });
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
