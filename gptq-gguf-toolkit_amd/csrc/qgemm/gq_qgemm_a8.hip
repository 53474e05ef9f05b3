// gq_qgemm_a8.hip -- K35: the packed-weight forward on int8 activations.
//   gq_quantize_act_q8   x [T, C] fp16 / bf16 -> codes int8 [T, C], a step fp32 per 256 values, group sums int16 per 16 values
//   gq_linear_packed_a8  y = x W^T from those and the packed blocks of W, on the int8 matrix pipe
// The contract of both is include/gptq_gguf_qgemm_a8.h's.  No weight is turned into a float here: a code becomes an int8
// operand with shifts and masks, the products of a scale group are summed exactly by one MFMA, the group's integer scale is
// applied to that int32 tile with one 24-bit multiply-add per element, and the float side (d, dmin, the activation step)
// happens once per superblock of 256 values.
//
// The quantizer.  32 lanes own a superblock: a lane loads 16 bytes (8 values), the maximum goes through five cross-lane
// exchanges, a lane stores its 8 codes as 8 bytes, two lanes make a group sum.  The [T, C] tensor is one run of T * C / 256
// superblocks, 8 to a workgroup; no loop, no workspace.
//
// The GEMM.  A workgroup of 4 waves owns [TT = 128 tokens, TR = 128 rows] and walks C in superblocks (K21's tiling and its
// LDS slots of the packed rows, QL<QT>; staged by stage_packed below).  Wave w owns rows 32 w .. 32 w + 31 and all 128 tokens as four
// 32 x 32 tiles.  The matrix instruction is v_mfma_i32_32x32x{16,32}_i8 with A = x and B = W, so that a lane's 16 results are
// D[token 8 (i >> 2) + 4 (l >> 5) + (i & 3)][row l & 31]: ONE weight row per lane.  Everything that belongs to a row -- its
// LDS slot, d, dmin, the group's scale -- is therefore one value per lane, read once, and the sub-scale step is
// v_mad_i32_i24(sc, D[i], isum[i]) with the same sc for all 16 registers.
//   * Q4_K, Q5_K, Q8_0 (groups of 32): 32x32x32, a lane's operand is 16 bytes = values 32 g + 16 (l >> 5) .. + 15 of its
//     row (codes16 as it stands) and of its token.  One MFMA per group.
//   * Q3_K, Q6_K (groups of 16): 32x32x16, 8 bytes = values 16 g + 8 (l >> 5) .. + 7.  One MFMA per group.
//   * Q2_K (groups of 16): 32x32x16 as well, but the scale is folded into the operand (sc w <= 15 * 3 = 45 fits a byte, one
//     32-bit multiply per word), so the sixteen MFMAs of a superblock chain through the accumulator and no VALU work follows
//     them.  Q3_K is not folded (a per-byte signed product is not one instruction) and Q6_K cannot be (|sc w| up to 4096).
//   * mins (Q2_K, Q4_K, Q5_K): msum = sum_g mn_g xbsum_g is itself a [rows, 16] x [16, tokens] integer product.  xbsum does not
//     fit a byte, so it is staged as two byte planes, xbsum = 64 hi + lo with lo in [0, 63] and hi in [-32, 31], and two
//     32x32x16 MFMAs per token tile and superblock give msum = 64 Dhi + Dlo.  The weight operand holds mn of the group that the
//     16-value group g16 lies in (Q4_K / Q5_K: each min twice).
//   * float side, per superblock and element: xd * (d * float(isum) - dmin * float(msum)); Q8_0 per block: fs += d_b * float(D).
// LDS: the packed slots (K21's), the superblock's xq tile [128 tokens, 256 bytes] at a pitch of 272 (16-byte reads) or 264
// bytes (8-byte reads) so that the 16 (32) tokens of a read fall on different banks, the two xbsum planes [128, 16] and xd:
// 51 KB (Q2_K) .. 78 KB (Q8_0), two workgroups per CU.  The next superblock's xq, xbsum and xd are loaded into registers
// while the MFMAs run.
// Edges: rows >= R are not staged (their slots hold stale bytes that only reach results which are never stored, a lane holds
// one row only), tokens >= T are staged as zeros and not stored.  y is written with 2-byte stores, 32 lanes = 64 contiguous
// bytes of one token's row of y: with one row per lane there are no four consecutive rows in a lane to store 8 bytes wide.
#include "../../../include/gptq_gguf_qgemm_a8.h"

#include "../search/gq_block_host.hpp"
#include "gq_qgemm_a8_core.hpp"

namespace gq {
namespace {

using namespace a8core;  // the tile's text and the quantizer's rule (shared with gq_moe_gemm_a8.hip)

// ------------------------------------------------------------------------------------------------ the quantizer
template <bool BF16>
__global__ __launch_bounds__(256) void quantize_act_q8_kernel(const uint16_t* __restrict__ x, int64_t nsb, int8_t* __restrict__ xq,
                                                              float* __restrict__ xd, int16_t* __restrict__ xbsum) {
    const int64_t sbi = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 5;
    const int piece = threadIdx.x & 31;
    const bool on = sbi < nsb;  // (a whole half wave is on or off: the exchanges stay inside it)
    uint4 raw = make_uint4(0, 0, 0, 0);
    if (on) raw = *reinterpret_cast<const uint4*>(x + sbi * 256 + piece * 8);
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint16_t b = (uint16_t)(w[k >> 1] >> (16 * (k & 1)));
        v[k] = BF16 ? bf2f(b) : h2f(b);
    }
    quantize_superblock(v, on, sbi, piece, xq, xd, xbsum);
}

// ------------------------------------------------------------------------------------------------ the GEMM
template <int QT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void linear_packed_a8_kernel(
    const uint8_t* __restrict__ blocks, const int32_t* __restrict__ row_src, int64_t R, int64_t C, const int8_t* __restrict__ xq,
    const float* __restrict__ xd, const int16_t* __restrict__ xbsum, int64_t T, uint16_t* __restrict__ y, int bf16, uint32_t n_rt) {
    using Q = QL<QT>;
    using L = TileLds<QT>;
    __shared__ __attribute__((aligned(16))) uint8_t sb[L::SB];
    __shared__ __attribute__((aligned(16))) uint8_t sx[L::SX];
    __shared__ __attribute__((aligned(16))) uint8_t sbl[L::PLANE], sbh[L::PLANE];
    __shared__ __attribute__((aligned(16))) float sxd[TT];
    __shared__ int64_t sbase[TR];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)(blockIdx.x % n_rt) * TR, t0 = (int64_t)(blockIdx.x / n_rt) * TT;  // row tiles fastest: they share x
    const int nr = (int)((R - r0) < TR ? (R - r0) : TR), nt = (int)((T - t0) < TT ? (T - t0) : TT), ntt = (nt + 31) >> 5;
    if (tid < nr) sbase[tid] = (row_src ? (int64_t)row_src[r0 + tid] : r0 + tid) * (C / 256) * Q::ROWB;
    auto row = [=](int i) { return t0 + i < T ? t0 + i : (int64_t)-1; };  // tile token i is token t0 + i of x and of y
    tile_pass_a8<QT>(blocks, sbase, nr, ntt, r0, R, C, xq, xd, xbsum, row, y, bf16, row, sb, sx, sbl, sbh, sxd);
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_quantize_act_q8(const void* x, int64_t T, int64_t C, int x_dtype, int8_t* xq, float* xd, int16_t* xbsum, void* stream) {
    if (int rc = options_ok()) return rc;
    const char* who = "gq_quantize_act_q8";
    if (x_dtype != GQ_F16 && x_dtype != GQ_BF16)
        GQ_FAIL(GQ_E_BAD_TYPE, "%s: x_dtype %d (GQ_F16 or GQ_BF16; there is no fp32 path)", who, x_dtype);
    if (int rc = need(who, "x", x)) return rc;
    if (int rc = need(who, "xq", xq)) return rc;
    if (int rc = need(who, "xd", xd)) return rc;
    if (int rc = need(who, "xbsum", xbsum)) return rc;
    if (T < 1 || T > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: T=%ld (not in [1, 2^31))", who, (long)T);
    if (int rc = check_C256(who, C)) return rc;
    const int64_t nsb = T * (C / 256), n_wg = (nsb + 7) / 8;
    if (n_wg > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: T=%ld C=%ld is more than one launch takes", who, (long)T, (long)C);
    if (int rc = check_aligned(who, "x", x, 16)) return rc;
    if (int rc = check_aligned(who, "xq", xq, 16)) return rc;
    if (int rc = check_aligned(who, "xd", xd, 16)) return rc;
    if (int rc = check_aligned(who, "xbsum", xbsum, 16)) return rc;
    hipStream_t st = (hipStream_t)stream;
    dispatch_bool(x_dtype == GQ_BF16, [&](auto bf16) {
        hipLaunchKernelGGL((quantize_act_q8_kernel<decltype(bf16)::value>), dim3((unsigned)n_wg), dim3(256), 0, st,
                           static_cast<const uint16_t*>(x), nsb, xq, xd, xbsum);
    });
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

int gq_linear_packed_a8(int q_type, const void* blocks, const int32_t* row_src, int64_t R, int64_t C, const int8_t* xq,
                        const float* xd, const int16_t* xbsum, int64_t T, void* y, int y_dtype, void* stream) {
    if (int rc = options_ok()) return rc;
    const char* who = "gq_linear_packed_a8";
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
    if (int rc = need(who, "y", y)) return rc;
    if (int rc = check_R(who, R)) return rc;
    if (T < 1 || T > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: T=%ld (not in [1, 2^31))", who, (long)T);
    if (int rc = check_C256(who, C)) return rc;
    if (int rc = check_blocks_aligned(who, q_type, blocks)) return rc;
    if (int rc = check_aligned(who, "row_src", row_src, 4)) return rc;
    if (int rc = check_aligned(who, "xq", xq, 16)) return rc;
    if (int rc = check_aligned(who, "xd", xd, 16)) return rc;
    if (int rc = check_aligned(who, "xbsum", xbsum, 16)) return rc;
    if (int rc = check_aligned(who, "y", y, 16)) return rc;
    const int64_t n_rt = (R + TR - 1) / TR, n_tt = (T + TT - 1) / TT;
    if (n_tt > 0x7fffffff / n_rt) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: R=%ld T=%ld is more than one launch takes", who, (long)R, (long)T);
    const dim3 grid((unsigned)(n_rt * n_tt));
    hipStream_t st = (hipStream_t)stream;
    dispatch_packed(q_type, [&](auto qt) {
        constexpr int QT = decltype(qt)::value;
        if constexpr (a8_type(QT))
            hipLaunchKernelGGL((linear_packed_a8_kernel<QT>), grid, dim3(256), 0, st, static_cast<const uint8_t*>(blocks), row_src, R,
                               C, xq, xd, xbsum, T, static_cast<uint16_t*>(y), (int)(y_dtype == GQ_BF16), (uint32_t)n_rt);
    });
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
