// gq_moe_gemv_a8.hip -- K38: the grouped expert GEMV of a packed MoE layer's decode step on int8 activations.
//   gq_gemv_packed_experts_a8  y[p] = W[pair_expert[p]] . Q8(x[p / pairs_per_row]) for the P <= 64 pairs of a step, one launch
//   gq_gemv_experts_a8_plan    the LDS image, the rows of a turn, the grid: csrc/qgemm/gq_gemv_a8_plan.hpp
// The contract is include/gptq_gguf_moe_gemv_a8.h's.  K37's form (gq_gemv_a8.hip: the activation quantizer in the prologue,
// weights straight into registers, v_dot4_i32_i8 against the image in LDS, integer reductions over four lanes) on K24's grid
// (gq_moe_gemv.hip: a second grid dimension over the experts and a device-side mask of the pairs).
//
// Grid (gx, E), 16 waves per workgroup.  Every wave of workgroup (b, e) reads the P <= 64 expert ids, one per lane, and
// ballots the mask of the pairs that name e: the same mask in every wave, so no LDS and no barrier is spent on it, and it
// lives in scalar registers.  A workgroup whose expert no pair names returns there -- before any load of a weight byte and
// before the prologue; ids outside [0, E) match no workgroup.  With Mixtral's E = 8, K = 2 and T = 1 six of eight rows of
// the grid return at once and 2 gx workgroups stream two experts' bytes; gx is capped (GEMV_EXPERTS_A8_GRID_X_CAP) and
// workgroup b walks row groups b, b + gx, .. of 16 rows, one row per wave, so an expert pays for at most gx prologues.
//
// A pass serves up to 4 matching pairs, in pair order: image token i is the i-th matching pair of the pass, its input row
// p / pairs_per_row gathered by the prologue (gemva8::quantize_image: a8core::quantize_superblock on 32 superblocks per turn,
// so token i's part of the image is byte for byte what gq_quantize_act_q8 writes for that row), its output row p scattered
// by the store.  Each wave issues the loads of its first weight row before the prologue; the barrier after the prologue is
// the only one of a pass.  An expert named by more than 4 pairs takes further passes: one more barrier (every wave has
// finished reading the image), the prologue again, the weight again.  A decode step with distinct experts per token and
// T <= 4 never has them; nothing relies on that.
//
// Tokens of a pass.  The count n is uniform over the workgroup but not over the grid, so the workgroup switches between the
// TT = 1 .. 4 instances of the walk: a T = 1 step (n = 1 everywhere) runs the instance without any idle column.  The other
// form -- one TT = 4 instance whose columns n .. 3 are computed on whatever LDS holds and not stored -- is kept behind
// GQ_GEMV_EXPERTS_A8_IDLE_COLUMNS for the A/B of profiles/moe_gemv_a8_rate.py: it is 1.2 - 1.9 x slower for Q2_K, Q3_K, Q4_K
// and Q6_K at every T and level (within 7 %) for Q5_K and Q8_0, the two types whose switch form spills (DESIGN K38).
//
// Fused SwiGLU (x_up != NULL, the down launch): the prologue's value is a8core::silu_mul_rounded(x, x_up), the text
// gq_silu_mul_quantize_act_q8 runs, so the image is byte for byte that call's output and the [P, I] 16-bit activation is
// never written.
//
// The row walk is gq_gemv_a8_core.hpp's, the text gq_gemv_packed_a8 runs, on expert e's slice: a token's accumulator is
// touched by no other token, so row p of y is bit for bit gq_gemv_packed_a8 at T = 1 on that slice and that input row.
// No atomics, no workspace, no scratch, no host synchronisation; y is written with plain vector stores.
#include "../../../include/gptq_gguf_moe_gemv_a8.h"

#include <atomic>

#include "../search/gq_block_host.hpp"
#include "gq_gemv_a8_core.hpp"
#include "gq_moe_lookup.hpp"

namespace gq {
namespace {

using namespace gemva8;
using moelookup::nth_set_bit;

// The prologue of a pass of workgroup (b, e): its n matching pairs as tokens 0 .. n - 1 of an image of T rows; byte i of xk is
// token i's row of x (P <= 64).
__device__ __forceinline__ void gather_image(int T, int n, int C, uint32_t xk, const uint16_t* __restrict__ x,
                                             const uint16_t* __restrict__ x_up, int bf16, uint8_t* a8_img) {
    const int nsb = C / 256;
    quantize_image(
        T, n * nsb, C,
        [=](int sbi) {  // image superblock sbi = superblock sbi - i nsb of token i
            int i = 0;
#pragma unroll
            for (int u = 1; u < GEMV_EXPERTS_A8_PASS; ++u) i += sbi >= u * nsb;
            const int row = (xk >> (8 * i)) & 0xffu;
            return ((int64_t)row * nsb + (sbi - i * nsb)) * 256;
        },
        x, x_up, bf16, a8_img);
}

template <int QT>
__global__ __launch_bounds__(NT) void gemv_packed_experts_a8_kernel(const uint8_t* __restrict__ blocks, int64_t R, int C,
                                                                   const uint16_t* __restrict__ x, const uint16_t* __restrict__ x_up,
                                                                   const int32_t* __restrict__ pair_expert, int P, int pairs_per_row,
                                                                   int bf16, uint16_t* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) uint8_t a8_img[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), p = lane & 3, g4 = lane >> 2;
    const int e = blockIdx.y;
    // bit q: pair q names this workgroup's expert (ids outside [0, E) match no workgroup: such a pair is skipped)
    const uint64_t m = __ballot(lane < P && pair_expert[lane] == e);
    if (m == 0) return;  // uniform over the workgroup: every wave read the same ids
    const int nm = __builtin_popcountll(m), nsb = C / 256;
    auto row_at = rows_of<QT>(blocks, [=](int64_t r) { return (int64_t)e * R + r; }, nsb);  // expert e's slice of the stacked tensor
    auto next = rows_apart((int64_t)gridDim.x * GEMV_A8_ROWS);
    for (int first = 0;;) {
        const int n = nm - first < GEMV_EXPERTS_A8_PASS ? nm - first : GEMV_EXPERTS_A8_PASS;
        const int64_t r = (int64_t)blockIdx.x * GEMV_A8_ROWS + wave;
        uint32_t cur[NRAW<QT>] = {};
        if (r < R) load_item<QT>(row_at, nsb, g4, p, cur, r, 0);  // in flight during the prologue
        uint32_t pk = 0, xk = 0;  // the pass's pairs and their rows of x, from the mask
        for (int i = 0; i < n; ++i) {
            const int q = nth_set_bit(m, first + i);
            pk |= (uint32_t)q << (8 * i), xk |= (uint32_t)(q / pairs_per_row) << (8 * i);
        }
        pk = __builtin_amdgcn_readfirstlane(pk), xk = __builtin_amdgcn_readfirstlane(xk);
        const int T = GEMV_EXPERTS_A8_IDLE_COLUMNS ? GEMV_EXPERTS_A8_PASS : n;  // tokens of the walk's instance = rows of the image
        gather_image(T, n, C, xk, x, x_up, bf16, a8_img);
        __syncthreads();
        // byte t of pk: the row of y of token t
        auto done = store_rows(y, R, bf16, [=](int t) { return t < n ? (int)((pk >> (8 * t)) & 0xffu) : -1; });
        switch (T) {
        case 1: row_walk<QT, 1>(row_at, R, C, r, next, cur, a8_img, done); break;
        case 2: row_walk<QT, 2>(row_at, R, C, r, next, cur, a8_img, done); break;
        case 3: row_walk<QT, 3>(row_at, R, C, r, next, cur, a8_img, done); break;
        default: row_walk<QT, 4>(row_at, R, C, r, next, cur, a8_img, done); break;
        }
        if ((first += GEMV_EXPERTS_A8_PASS) >= nm) return;
        __syncthreads();  // every wave has finished reading the image: the next pass may write it
    }
}

template <int QT>
int launch(const GemvExpertsA8Plan& pl, const uint8_t* blocks, int64_t E, int64_t R, int64_t C, const uint16_t* x, const uint16_t* x_up,
           const int32_t* pair_expert, int64_t P, int64_t pairs_per_row, int bf16, uint16_t* y, hipStream_t st) {
    static std::atomic<bool> attr_set{false};
    if (!attr_set) {
        GQ_HIP(hipFuncSetAttribute((const void*)gemv_packed_experts_a8_kernel<QT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)GEMV_A8_LDS_BUDGET));
        attr_set = true;
    }
    hipLaunchKernelGGL((gemv_packed_experts_a8_kernel<QT>), dim3((unsigned)pl.grid_x, (unsigned)E), dim3(NT), (size_t)pl.lds_bytes, st,
                       blocks, R, (int)C, x, x_up, pair_expert, (int)P, (int)pairs_per_row, bf16, y);
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

int check_P(const char* who, int64_t P) {
    if (P < 1 || P > GQ_MOE_MAX_PAIRS) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: P=%ld (not in [1, %d] pairs)", who, (long)P, GQ_MOE_MAX_PAIRS);
    return GQ_OK;
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_gemv_experts_a8_plan(int64_t P, int64_t R, int64_t C, int64_t* lds_bytes, int64_t* rows_per_turn, int64_t* grid_x_cap,
                            int64_t* grid_x, int64_t* fits) {
    const char* who = "gq_gemv_experts_a8_plan";
    if (int rc = check_P(who, P)) return rc;
    if (int rc = check_R(who, R)) return rc;
    if (int rc = check_C256(who, C)) return rc;
    const GemvExpertsA8Plan p = make_gemv_experts_a8_plan(P, R, C);
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    if (rows_per_turn) *rows_per_turn = p.rows_per_turn;
    if (grid_x_cap) *grid_x_cap = p.grid_x_cap;
    if (grid_x) *grid_x = p.grid_x;
    if (fits) *fits = p.fits;
    return GQ_OK;
}

int gq_gemv_packed_experts_a8(int q_type, const void* blocks, int64_t E, int64_t R, int64_t C, const void* x, const void* x_up,
                              int64_t x_rows, const int32_t* pair_expert, int64_t P, int64_t pairs_per_row, int x_dtype, void* y,
                              void* stream) {
    if (int rc = options_ok()) return rc;
    const char* who = "gq_gemv_packed_experts_a8";
    if (q_type == GQ_IQ4_NL || q_type == GQ_IQ4_XS)
        GQ_FAIL(GQ_E_BAD_TYPE, "%s: q_type %d (%s) is not served on int8 activations (a K-quant or GQ_Q8_0)", who, q_type,
                q_type == GQ_IQ4_NL ? "GQ_IQ4_NL" : "GQ_IQ4_XS");
    if (!a8_type(q_type)) GQ_FAIL(GQ_E_BAD_TYPE, "%s: unknown q_type %d (a K-quant or GQ_Q8_0)", who, q_type);
    if (int rc = check_types(who, q_type, x_dtype)) return rc;
    if (int rc = need(who, "blocks", blocks)) return rc;
    if (int rc = need(who, "x", x)) return rc;
    if (int rc = need(who, "pair_expert", pair_expert)) return rc;
    if (int rc = need(who, "y", y)) return rc;
    if (E < 1 || E > 65535) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: E=%ld (not in [1, 65535])", who, (long)E);
    if (int rc = check_R(who, R)) return rc;
    if (int rc = check_P(who, P)) return rc;
    if (int rc = check_pairs(who, x_rows, pairs_per_row, P)) return rc;
    if (int rc = check_C256(who, C)) return rc;
    const GemvExpertsA8Plan pl = make_gemv_experts_a8_plan(P, R, C);
    if (!pl.fits)
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: P=%ld C=%ld: the quantized image of %ld rows of x, %ld bytes, does not fit the %ld bytes of LDS it may take",
                who, (long)P, (long)C, (long)pl.image_rows, (long)pl.lds_bytes, (long)GEMV_A8_LDS_BUDGET);
    if (int rc = check_blocks_aligned(who, q_type, blocks)) return rc;
    if (int rc = check_aligned(who, "pair_expert", pair_expert, 4)) return rc;
    if (int rc = check_aligned(who, "x", x, 16)) return rc;
    if (int rc = check_aligned(who, "x_up", x_up, 16)) return rc;
    if (int rc = check_aligned(who, "y", y, 16)) return rc;
    int rc = GQ_OK;
    dispatch_packed(q_type, [&](auto qt) {
        constexpr int QT = decltype(qt)::value;
        if constexpr (a8_type(QT))
            rc = launch<QT>(pl, static_cast<const uint8_t*>(blocks), E, R, C, static_cast<const uint16_t*>(x),
                            static_cast<const uint16_t*>(x_up), pair_expert, P, pairs_per_row, (int)(x_dtype == GQ_BF16),
                            static_cast<uint16_t*>(y), (hipStream_t)stream);
    });
    return rc;
}

}  // extern "C"
