// gq_gemv_a8.hip -- K37: the decode step of a packed model on int8 activations.
//   gq_gemv_packed_a8  y = x W^T for 1 <= T <= 4 tokens: x is quantized to the Q8 activation format inside the kernel and
//                      multiplied with the integer codes of the packed weight on the VALU's 4 x int8 dot product
//   gq_gemv_a8_plan    the LDS image, the rows of a turn, the grid: csrc/qgemm/gq_gemv_a8_plan.hpp
// The contract is include/gptq_gguf_qgemv_a8.h's.  No weight becomes a float and no matrix instruction is issued: at T <= 4
// an MFMA tile is at least three quarters empty, while v_dot4_i32_i8 does four multiply-adds per lane and needs only the
// shifts and masks that turn the stored bits into bytes.
//
// Prologue.  A workgroup of 16 waves quantizes the T rows of x once into LDS with a8core::quantize_superblock -- the text
// gq_quantize_act_q8 runs, so the image [codes T C | group sums of 16, int16, T C / 8 | steps, fp32, T C / 64] is byte for
// byte what that call writes -- 32 superblocks per pass.  The grid is capped at one workgroup per CU and a workgroup walks row
// groups b, b + grid, .. so that lm_head's > 100 k rows pay for 256 prologues, not 8000.  A wave issues the loads of its
// first row BEFORE the prologue; the barrier after the prologue is the only one of the kernel.
//
// Work split.  A wave owns one row per turn (16 rows per workgroup and turn) and all of C: no K split across waves, no LDS
// reduction.  Four lanes own one superblock of the row, 64 values each, so the 64 lanes of a wave cover 16 consecutive
// superblocks = one contiguous run of the row's bytes per step (all of a 4096-column row at once).  A lane loads its piece of
// the block STRAIGHT INTO REGISTERS (no LDS staging of weights), unpacks it once into sixteen 4 x int8 operands and reuses
// them for every token against xq read from LDS (ds_read_b128, 64 bytes per token).  The next step's pieces are in flight
// while this one's dot products run.  What a lane holds of superblock j, lane p = 0 .. 3 of its group:
//   Q4_K / Q5_K  the 64-value chunk p: qs[32 p .. + 31] (Q5_K: and all of qh), i.e. groups 2 p and 2 p + 1 whole; the 16
//                header bytes in every lane (one address per group: a broadcast)
//   Q2_K / Q3_K / Q6_K  half ch = p >> 1 of the superblock, bytes l0 = 16 (p & 1) .. + 15 of its 32-byte planes: quarter k of
//                those bytes is the whole 16-value group 8 ch + 2 k + (p & 1), values 128 ch + 32 k + l0 .. + 15
//   Q8_0         blocks 2 p and 2 p + 1, 68 contiguous bytes: two d and two runs of 32 codes
// so every lane holds whole scale groups: a group's products are summed by four (eight) dot4, multiplied by the integer
// scale and added up in the lane; isum and msum = sum mn_g xbsum_g are then reduced over the four lanes AS INTEGERS (two
// exchanges each) -- exact.  Every lane of the group computes the contract's fp32 sequence xd (d float(isum) - dmin float(msum))
// (Q8_0: d_b float(isum_b) per block, summed pairwise over the eight blocks) and adds it to its accumulator of that token; at
// the end of the row the sixteen lane groups are summed by a binary tree of exchanges and lane t stores token t, rounded once.
//
// 2-byte aligned types (Q3_K 110 B, Q6_K 210 B, Q8_0 8 x 34 B).  A piece of n dwords at a 2-byte aligned address a with
// a % 4 == 2 is fetched as [2 bytes at a][n - 1 aligned dwords from a + 2][2 bytes at a + 4 n - 2] and put together with
// v_alignbyte; with a % 4 == 0 it is n aligned dwords.  Exactly the piece's bytes either way: nothing before the first block
// or after the last is touched, wherever the buffer begins.  (K22: 14 - 34 two-byte loads per lane and superblock.)
#include "../../../include/gptq_gguf_qgemv_a8.h"

#include <atomic>

#include "../search/gq_block_host.hpp"
#include "gq_gemv_a8_core.hpp"

namespace gq {
namespace {

using namespace gemva8;  // piece, load_raw, lane_dots, row_walk: the text gq_moe_gemv_a8.hip (K38) runs too

template <int QT, int TT>
__global__ __launch_bounds__(NT) void gemv_packed_a8_kernel(const uint8_t* __restrict__ blocks, const int32_t* __restrict__ row_src,
                                                           int64_t R, int C, const uint16_t* __restrict__ x, int bf16,
                                                           uint16_t* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) uint8_t a8_img[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), p = lane & 3, g4 = lane >> 2;
    const int nsb = C / 256;
    auto row_at = rows_of<QT>(blocks, [=](int64_t r) { return row_src ? (int64_t)row_src[r] : r; }, nsb);

    const int64_t r = (int64_t)blockIdx.x * GEMV_A8_ROWS + wave;
    uint32_t cur[NRAW<QT>] = {};
    if (r < R) load_item<QT>(row_at, nsb, g4, p, cur, r, 0);  // in flight during the prologue

    // ---- the prologue: x -> the image; the T rows of x are the image's superblocks in order
    quantize_image(TT, TT * nsb, C, [](int sbi) { return (int64_t)sbi * 256; }, x, nullptr, bf16, a8_img);
    __syncthreads();

    row_walk<QT, TT>(row_at, R, C, r, rows_apart((int64_t)gridDim.x * GEMV_A8_ROWS), cur, a8_img,
                     store_rows(y, R, bf16, [](int t) { return t; }));
}

template <int QT, int TT>
int launch(const GemvA8Plan& pl, const uint8_t* blocks, const int32_t* row_src, int64_t R, int64_t C, const uint16_t* x, int bf16,
           uint16_t* y, hipStream_t st) {
    static std::atomic<bool> attr_set{false};
    if (!attr_set) {
        GQ_HIP(hipFuncSetAttribute((const void*)gemv_packed_a8_kernel<QT, TT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)GEMV_A8_LDS_BUDGET));
        attr_set = true;
    }
    hipLaunchKernelGGL((gemv_packed_a8_kernel<QT, TT>), dim3((unsigned)pl.grid), dim3(NT), (size_t)pl.lds_bytes, st, blocks, row_src, R,
                       (int)C, x, bf16, y);
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_gemv_a8_plan(int64_t T, int64_t R, int64_t C, int64_t* lds_bytes, int64_t* rows_per_turn, int64_t* grid_cap, int64_t* grid,
                    int64_t* fits) {
    const char* who = "gq_gemv_a8_plan";
    if (T < 1 || T > GQ_GEMV_A8_MAX_T) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: T=%ld (not in [1, %d])", who, (long)T, GQ_GEMV_A8_MAX_T);
    if (int rc = check_R(who, R)) return rc;
    if (int rc = check_C256(who, C)) return rc;
    const GemvA8Plan p = make_gemv_a8_plan(T, R, C);
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    if (rows_per_turn) *rows_per_turn = p.rows_per_turn;
    if (grid_cap) *grid_cap = p.grid_cap;
    if (grid) *grid = p.grid;
    if (fits) *fits = p.fits;
    return GQ_OK;
}

int gq_gemv_packed_a8(int q_type, const void* blocks, const int32_t* row_src, int64_t R, int64_t C, const void* x, int64_t T,
                      int x_dtype, void* y, void* stream) {
    if (int rc = options_ok()) return rc;
    const char* who = "gq_gemv_packed_a8";
    if (q_type == GQ_IQ4_NL || q_type == GQ_IQ4_XS)
        GQ_FAIL(GQ_E_BAD_TYPE, "%s: q_type %d (%s) is not served on int8 activations (a K-quant or GQ_Q8_0)", who, q_type,
                q_type == GQ_IQ4_NL ? "GQ_IQ4_NL" : "GQ_IQ4_XS");
    if (!a8_type(q_type)) GQ_FAIL(GQ_E_BAD_TYPE, "%s: unknown q_type %d (a K-quant or GQ_Q8_0)", who, q_type);
    if (int rc = check_types(who, q_type, x_dtype)) return rc;
    if (int rc = need(who, "blocks", blocks)) return rc;
    if (int rc = need(who, "x", x)) return rc;
    if (int rc = need(who, "y", y)) return rc;
    if (int rc = check_R(who, R)) return rc;
    if (T < 1 || T > GQ_GEMV_A8_MAX_T)
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: T=%ld (not in [1, %d]; gq_gemv_packed takes up to %d tokens)", who, (long)T, GQ_GEMV_A8_MAX_T,
                GQ_GEMV_MAX_T);
    if (int rc = check_C256(who, C)) return rc;
    const GemvA8Plan pl = make_gemv_a8_plan(T, R, C);
    if (!pl.fits)
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: T=%ld C=%ld: the quantized image of x, %ld bytes, does not fit the %ld bytes of LDS it may take",
                who, (long)T, (long)C, (long)pl.lds_bytes, (long)GEMV_A8_LDS_BUDGET);
    if (int rc = check_blocks_aligned(who, q_type, blocks)) return rc;
    if (int rc = check_aligned(who, "row_src", row_src, 4)) return rc;
    if (int rc = check_aligned(who, "x", x, 16)) return rc;
    if (int rc = check_aligned(who, "y", y, 16)) return rc;
    int rc = GQ_OK;
    dispatch_packed(q_type, [&](auto qt) {
        constexpr int QT = decltype(qt)::value;
        if constexpr (a8_type(QT)) {
            auto go = [&](auto tt) {
                rc = launch<QT, decltype(tt)::value>(pl, static_cast<const uint8_t*>(blocks), row_src, R, C, static_cast<const uint16_t*>(x),
                                                     (int)(x_dtype == GQ_BF16), static_cast<uint16_t*>(y), (hipStream_t)stream);
            };
            switch (T) {
            case 1: go(std::integral_constant<int, 1>{}); break;
            case 2: go(std::integral_constant<int, 2>{}); break;
            case 3: go(std::integral_constant<int, 3>{}); break;
            default: go(std::integral_constant<int, 4>{}); break;
            }
        }
    });
    return rc;
}

}  // extern "C"
