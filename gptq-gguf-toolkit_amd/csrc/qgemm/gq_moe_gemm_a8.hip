// gq_moe_gemm_a8.hip -- K36: the prefill of a packed MoE layer on int8 activations.
//   gq_linear_packed_experts_a8   every (token, expert) pair of gq_moe_route's order times its expert's packed weight, on the
//                                 int8 matrix pipe, in one launch
//   gq_silu_mul_quantize_act_q8   silu(gate) * up written as quantized activations: the input of the down launch
// The contract of both is include/gptq_gguf_moe_gemm_a8.h's.
//
// The GEMM.  K loop, staging and epilogue are gq_qgemm_a8_core.hpp's tile_pass_a8, the text gq_linear_packed_a8 runs (K35, its
// form is described at the head of gq_qgemm_a8.hip): a workgroup of 4 waves owns [128 pairs of one expert, 128 rows].  What is
// this kernel's own:
//   * grid and lookup are K25's: n_rt x (ceil(P / 128) + min(E, P)) workgroups, row tiles fastest (they share the expert and
//     its pairs); every wave finds (expert, tile) from expert_start with a wave-wide scan and a ballot (gq_moe_lookup.hpp), a
//     workgroup without work returns before any staging.
//   * the gather costs no persistent register.  K35's instances sit at 228-250 VGPRs at two waves per SIMD, so K25's way --
//     the gathered row indices of a thread's loads held in registers through the K loop -- has no room.  The tile's gather
//     list is written ONCE, before the K loop, into 1 KB of LDS: 128 x int32 activation rows (pair / pairs_per_row, or -1) and
//     128 x int32 rows of y (the pair, or -1).  The prefetch of a superblock reads a token's row back from LDS (a broadcast
//     read of 16 lanes per address) and the xq, xbsum and xd loads all address through it; the epilogue reads the y rows.
//     A token whose entry is -1 is staged as zeros, as a token beyond T is in K35.
//   * runs are short (T = 64, K = 2, E = 8: 7 - 22 pairs), so ntt = ceil(cnt / 32) matters more than in K35: the empty
//     32-token quarters of a tile issue no matrix instruction, no float side and no store.
//   * the epilogue keeps K35's 2-byte stores, 32 lanes = 64 contiguous bytes of a pair's row at pair * R.
// LDS: K35's plus the list, 54 784 (Q2_K) .. 76 288 B (Q8_0): two workgroups per CU (160 KB).
//
// The fused quantizer.  gq_quantize_act_q8's lane layout -- 32 lanes own a superblock, a lane loads 16 bytes of EACH input,
// five cross-lane exchanges for the maximum, 8-byte code stores, lane pairs make a group sum -- with gq_fwd_silu_mul's two
// roundings in front of quantize_superblock, the quantizer's own rule.  No LDS, no workspace, one launch.
#include "../../../include/gptq_gguf_moe_gemm_a8.h"

#include <math.h>

#include "../search/gq_block_host.hpp"
#include "gq_moe_lookup.hpp"
#include "gq_qgemm_a8_core.hpp"

namespace gq {
namespace {

using namespace a8core;
using namespace moelookup;

template <int QT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void linear_packed_experts_a8_kernel(
    const uint8_t* __restrict__ blocks, int E, int64_t R, int64_t C, const int8_t* __restrict__ xq, const float* __restrict__ xd,
    const int16_t* __restrict__ xbsum, int pairs_per_row, const int32_t* __restrict__ expert_start,
    const int32_t* __restrict__ order, int P, uint16_t* __restrict__ y, int bf16, uint32_t n_rt) {
    using Q = QL<QT>;
    using L = TileLds<QT>;
    __shared__ __attribute__((aligned(16))) uint8_t sb[L::SB];
    __shared__ __attribute__((aligned(16))) uint8_t sx[L::SX];
    __shared__ __attribute__((aligned(16))) uint8_t sbl[L::PLANE], sbh[L::PLANE];
    __shared__ __attribute__((aligned(16))) float sxd[TT];
    __shared__ int64_t sbase[TR];
    __shared__ __attribute__((aligned(16))) int32_t sxrow[TT], syrow[TT];  // the gather list: activation row and y row of a tile token
    const int tid = threadIdx.x;
    const int b = blockIdx.x / n_rt;  // row tiles fastest: they share the expert and its pairs
    int e, pos0, cnt;                 // this workgroup's (expert, tile)
    if (!expert_tile<TT>(expert_start, E, b, tid & 63, e, pos0, cnt)) return;  // uniform over the workgroup
    const int64_t r0 = (int64_t)(blockIdx.x % n_rt) * TR;
    const int nr = (int)((R - r0) < TR ? (R - r0) : TR), ntt = (cnt + 31) >> 5;
    if (tid < nr) sbase[tid] = ((int64_t)e * R + r0 + tid) * (C / 256) * Q::ROWB;
    if (tid < TT) {  // a position outside [0, P) and an entry outside [0, P) are never followed
        const int at = pos0 + tid;
        int p = tid < cnt && (unsigned)at < (unsigned)P ? order[at] : -1;
        if ((unsigned)p >= (unsigned)P) p = -1;
        syrow[tid] = p;
        sxrow[tid] = p < 0 ? -1 : p / pairs_per_row;
    }
    __syncthreads();  // the list is read by the first prefetch
    tile_pass_a8<QT>(
        blocks, sbase, nr, ntt, r0, R, C, xq, xd, xbsum, [&](int i) { return (int64_t)sxrow[i]; }, y, bf16,
        [&](int i) { return (int64_t)syrow[i]; }, sb, sx, sbl, sbh, sxd);
}

template <bool BF16>
__global__ __launch_bounds__(256) void silu_mul_quantize_act_q8_kernel(const uint16_t* __restrict__ gate, const uint16_t* __restrict__ up,
                                                                       int64_t nsb, int8_t* __restrict__ xq, float* __restrict__ xd,
                                                                       int16_t* __restrict__ xbsum) {
    const int64_t sbi = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 5;
    const int piece = threadIdx.x & 31;
    const bool on = sbi < nsb;  // (a whole half wave is on or off: the exchanges stay inside it)
    uint4 g4 = make_uint4(0, 0, 0, 0), u4 = g4;
    if (on) {
        g4 = *reinterpret_cast<const uint4*>(gate + sbi * 256 + piece * 8);
        u4 = *reinterpret_cast<const uint4*>(up + sbi * 256 + piece * 8);
    }
    const uint32_t G[4] = {g4.x, g4.y, g4.z, g4.w}, U[4] = {u4.x, u4.y, u4.z, u4.w};
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint16_t gb = (uint16_t)(G[k >> 1] >> (16 * (k & 1))), ub = (uint16_t)(U[k >> 1] >> (16 * (k & 1)));
        v[k] = silu_mul_rounded<BF16>(BF16 ? bf2f(gb) : h2f(gb), BF16 ? bf2f(ub) : h2f(ub));
    }
    quantize_superblock(v, on, sbi, piece, xq, xd, xbsum);
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_linear_packed_experts_a8(int q_type, const void* blocks, int64_t E, int64_t R, int64_t C, const int8_t* xq, const float* xd,
                                const int16_t* xbsum, int64_t x_rows, int64_t pairs_per_row, const int32_t* expert_start,
                                const int32_t* order, int64_t P, void* y, int y_dtype, void* stream) {
    if (int rc = options_ok()) return rc;
    const char* who = "gq_linear_packed_experts_a8";
    if (q_type == GQ_IQ4_NL || q_type == GQ_IQ4_XS)
        GQ_FAIL(GQ_E_BAD_TYPE, "%s: q_type %d (%s) is not served on int8 activations (a K-quant or GQ_Q8_0)", who, q_type,
                q_type == GQ_IQ4_NL ? "GQ_IQ4_NL" : "GQ_IQ4_XS");
    if (!a8_type(q_type)) GQ_FAIL(GQ_E_BAD_TYPE, "%s: unknown q_type %d (a K-quant or GQ_Q8_0)", who, q_type);
    if (y_dtype != GQ_F16 && y_dtype != GQ_BF16)
        GQ_FAIL(GQ_E_BAD_TYPE, "%s: y_dtype %d (GQ_F16 or GQ_BF16; there is no fp32 path)", who, y_dtype);
    if (int rc = need(who, "blocks", blocks)) return rc;
    if (int rc = need(who, "xq", xq)) return rc;
    if (int rc = need(who, "xd", xd)) return rc;
    if (int rc = need(who, "xbsum", xbsum)) return rc;
    if (int rc = need(who, "expert_start", expert_start)) return rc;
    if (int rc = need(who, "order", order)) return rc;
    if (int rc = need(who, "y", y)) return rc;
    if (E < 1 || E > GQ_MOE_ROUTE_MAX_EXPERTS)
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: E=%ld (not in [1, %d] experts)", who, (long)E, GQ_MOE_ROUTE_MAX_EXPERTS);
    if (int rc = check_R(who, R)) return rc;
    if (P < 1 || P > GQ_MOE_ROUTE_MAX_PAIRS)
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: P=%ld (not in [1, %d] pairs)", who, (long)P, GQ_MOE_ROUTE_MAX_PAIRS);
    if (int rc = check_pairs(who, x_rows, pairs_per_row, P)) return rc;
    if (int rc = check_C256(who, C)) return rc;
    if (int rc = check_blocks_aligned(who, q_type, blocks)) return rc;
    if (int rc = check_aligned(who, "expert_start", expert_start, 4)) return rc;
    if (int rc = check_aligned(who, "order", order, 4)) return rc;
    if (int rc = check_aligned(who, "xq", xq, 16)) return rc;
    if (int rc = check_aligned(who, "xd", xd, 16)) return rc;
    if (int rc = check_aligned(who, "xbsum", xbsum, 16)) return rc;
    if (int rc = check_aligned(who, "y", y, 16)) return rc;
    const int64_t n_rt = (R + TR - 1) / TR, n_tt = (P + TT - 1) / TT + (E < P ? E : P);  // n_tt <= 2^10 + 2^8
    if (n_rt > 0x7fffffff / n_tt) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: R=%ld P=%ld is more than one launch takes", who, (long)R, (long)P);
    const dim3 grid((unsigned)(n_rt * n_tt));
    hipStream_t st = (hipStream_t)stream;
    dispatch_packed(q_type, [&](auto qt) {
        constexpr int QT = decltype(qt)::value;
        if constexpr (a8_type(QT))
            hipLaunchKernelGGL((linear_packed_experts_a8_kernel<QT>), grid, dim3(256), 0, st, static_cast<const uint8_t*>(blocks), (int)E,
                               R, C, xq, xd, xbsum, (int)pairs_per_row, expert_start, order, (int)P, static_cast<uint16_t*>(y),
                               (int)(y_dtype == GQ_BF16), (uint32_t)n_rt);
    });
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

int gq_silu_mul_quantize_act_q8(const void* gate, const void* up, int64_t P, int64_t I, int dtype, int8_t* xq, float* xd,
                                int16_t* xbsum, void* stream) {
    if (int rc = options_ok()) return rc;
    const char* who = "gq_silu_mul_quantize_act_q8";
    if (dtype != GQ_F16 && dtype != GQ_BF16)
        GQ_FAIL(GQ_E_BAD_TYPE, "%s: dtype %d (GQ_F16 or GQ_BF16; there is no fp32 path)", who, dtype);
    if (int rc = need(who, "gate", gate)) return rc;
    if (int rc = need(who, "up", up)) return rc;
    if (int rc = need(who, "xq", xq)) return rc;
    if (int rc = need(who, "xd", xd)) return rc;
    if (int rc = need(who, "xbsum", xbsum)) return rc;
    if (P < 1 || P > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: P=%ld (not in [1, 2^31))", who, (long)P);
    if (I < 256 || I > 0x7fffffff || I % 256) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: I=%ld (I %% 256 != 0 or not in [256, 2^31))", who, (long)I);
    const int64_t nsb = P * (I / 256), n_wg = (nsb + 7) / 8;
    if (n_wg > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: P=%ld I=%ld is more than one launch takes", who, (long)P, (long)I);
    if (int rc = check_aligned(who, "gate", gate, 16)) return rc;
    if (int rc = check_aligned(who, "up", up, 16)) return rc;
    if (int rc = check_aligned(who, "xq", xq, 16)) return rc;
    if (int rc = check_aligned(who, "xd", xd, 16)) return rc;
    if (int rc = check_aligned(who, "xbsum", xbsum, 16)) return rc;
    hipStream_t st = (hipStream_t)stream;
    dispatch_bool(dtype == GQ_BF16, [&](auto bf16) {
        hipLaunchKernelGGL((silu_mul_quantize_act_q8_kernel<decltype(bf16)::value>), dim3((unsigned)n_wg), dim3(256), 0, st,
                           static_cast<const uint16_t*>(gate), static_cast<const uint16_t*>(up), nsb, xq, xd, xbsum);
    });
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
