// gq_qgemm.hip -- K21: y = x W^T for a Linear whose weight [R, C] exists only as GGUF block bytes (K-quants, Q8_0,
// IQ4_NL, IQ4_XS).
// gq_linear_packed is the forward of packed residency: the search and ppleval keep every level packed and no dense copy.
//
// Regime: T >= 256 tokens per call (calibration batches of the search, perplexity windows); small T is correct, not fast.
// Both operands are K-contiguous -- x rows and W rows --, so with v_mfma_f32_16x16x32_{f16,bf16} and A = W, B = x a lane's two
// fragments are each 8 consecutive k (16 bytes) of one row: lane l holds W[r = l & 15][8 (l >> 4) + j] and
// x[t = l & 15][8 (l >> 4) + j]; D[r = 4 (l >> 4) + i][t = l & 15] in register i.
//
// A workgroup of 4 waves owns the output tile [TT tokens, TR = 128 rows] and walks C in whole superblocks of 256.  TT = 256
// when that grid has at least 512 workgroups (two per CU), else TT = 128 (measured: the wide tile is 15-35 % faster where it
// fills the device and 15-25 % slower at [4096 x C] x 2048 tokens, 256 workgroups); the figures below are TT = 256's.
//   * the 128 rows' packed bytes of the superblock are staged in LDS with loads of the type's natural alignment that cover
//     exactly the blocks' bytes (as blockdec::stage_blocks), one slot per row;
//   * x is staged in four chunks of 64 k ([256, 64], 32 KB), the next chunk's global loads in flight during the MFMAs;
//   * wave w owns rows 32 w .. 32 w + 31 (two 16-row tiles) and all 256 tokens (sixteen tiles): 128 accumulator registers.
//     Per chunk a lane decodes, for each of its two rows, the 16 consecutive values 64 c + 16 (l >> 4) .. + 15 with
//     block_d / group_scale / codes16 / dequantize1 / cvt_out -- the text of decode_turn, so the operand bits are
//     gq_dequantize_blocks' -- and uses values 8 s .. 8 s + 7 as its fragment of MFMA step s = 0, 1.  (The k order
//     inside a chunk is thus permuted, identically for both operands.)  Only the wave that owns a row decodes it: a weight
//     is decoded once per workgroup and used 256 times (the decode is VALU work on the critical path: at a token tile
//     of 128 it weighs twice as much); no decoded [rows, K] tile exists anywhere.
// LDS: x chunk as 8 planes (one per 8-k piece u = 2 (l >> 4) + s) of 256 slots of 16 bytes: the 16 lanes of a quarter wave
// read 256 contiguous bytes, and the lane groups of ds_read_b128 ({0-3, 12-15, 20-27}, ...) take slots {0-3, 12-15} of one
// plane and {4-11} of another, planes 4096 bytes apart: conflict-free.  Packed slots have an odd number of 16-byte units
// (Q2_K / Q3_K 112, Q4_K / IQ4_NL / IQ4_XS 144, Q5_K 176, Q6_K 240, Q8_0 304 bytes) so that 16 rows' reads at the same offset fall on 16
// different 16-byte bank groups.  Budget: 32 KB + 128 slots + 1 KB of row offsets = 47 KB (Q2_K) .. 63 KB (Q6_K), 71 KB (Q8_0): two workgroups
// per CU, which is also what ~220 VGPRs allow; the staging latency of one is covered by the MFMAs of the other.
// Rows >= R and tokens >= T of an edge tile: the rows are not staged (their LDS slots hold stale bytes, decoded to values
// that only reach output elements that are never stored), the tokens are staged as zeros; nothing is read or written
// outside the arguments' extents.
#include "../../../include/gptq_gguf_qgemm.h"

#include "../search/gq_block_host.hpp"
#include "gq_qgemm_core.hpp"

namespace gq {
namespace {

using namespace gemmcore;  // the tile's text: staging, K loop, epilogue (shared with gq_moe_gemm.hip)

template <int QT, bool BF16, int TT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void linear_packed_kernel(const uint8_t* __restrict__ blocks, const int32_t* __restrict__ row_src,
                                                            int64_t R, int64_t C, const uint8_t* __restrict__ x, int64_t T,
                                                            uint16_t* __restrict__ y, uint32_t n_rt) {
    using Q = QL<QT>;
    __shared__ __attribute__((aligned(16))) uint8_t sb[TR * Q::SLOT];
    __shared__ __attribute__((aligned(16))) uint8_t sx[TT * KC * 2];
    __shared__ int64_t sbase[TR];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)(blockIdx.x % n_rt) * TR, t0 = (int64_t)(blockIdx.x / n_rt) * TT;  // row tiles fastest: they share x
    const int nr = (int)((R - r0) < TR ? (R - r0) : TR), nt = (int)((T - t0) < TT ? (T - t0) : TT), ntt = (nt + 15) >> 4;
    const int64_t nsb = C / 256;
    if (tid < nr) sbase[tid] = (row_src ? (int64_t)row_src[r0 + tid] : r0 + tid) * nsb * Q::ROWB;
    tile_pass<QT, BF16, TT>(
        blocks, sbase, nr, ntt, r0, R, C, x,
        [=](int i) {
            const int p = threadIdx.x + 256 * i;
            const int64_t t = t0 + (p >> 3);
            return Row{t < T, t};
        },
        y,
        [=](int tt) {
            const int64_t t = t0 + 16 * tt + (tid & 15);
            return Row{t < T, t};
        },
        sb, sx);
}

// the grid of token tile tt; 0 when it is more than one launch takes
int64_t tiles(int64_t R, int64_t T, int tt) {
    const int64_t n_rt = (R + TR - 1) / TR, n_tt = (T + tt - 1) / tt;
    return n_tt > 0x7fffffff / n_rt ? 0 : n_rt * n_tt;
}

// IQ4_XS has the 128-token tile only: its 256-token instance spills 190 bytes per lane inside the K loop and was measured at
// 1.7-2.3x Q4_K's time where the grid takes the wide tile, against 0.85-0.98x at the narrow one (DESIGN K26).
constexpr bool wide_ok(int q_type) { return q_type != GQ_IQ4_XS; }

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_linear_packed(int q_type, const void* blocks, const int32_t* row_src, int64_t R, int64_t C, const void* x, int64_t T,
                     int x_dtype, void* y, void* stream) {
    if (int rc = options_ok()) return rc;
    const char* who = "gq_linear_packed";
    if (int rc = check_types(who, q_type, x_dtype)) return rc;
    if (int rc = need(who, "blocks", blocks)) return rc;
    if (int rc = need(who, "x", x)) return rc;
    if (int rc = need(who, "y", y)) return rc;
    if (int rc = check_R(who, R)) return rc;
    if (T < 1 || T > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_linear_packed: T=%ld (not in [1, 2^31))", (long)T);
    if (int rc = check_C256(who, C)) return rc;
    if (int rc = check_blocks_aligned(who, q_type, blocks)) return rc;
    if (int rc = check_aligned(who, "row_src", row_src, 4)) return rc;
    if (int rc = check_aligned(who, "x", x, 16)) return rc;
    if (int rc = check_aligned(who, "y", y, 16)) return rc;
    // the 256-token tile halves the decode work per output, the 128-token one fills the device at small shapes
    const bool wide = wide_ok(q_type) && tiles(R, T, 256) >= WIDE_TILES;
    const int64_t n_rt = (R + TR - 1) / TR, n_wg = tiles(R, T, wide ? 256 : 128);
    if (!n_wg) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_linear_packed: R=%ld T=%ld is more than one launch takes", (long)R, (long)T);
    const dim3 grid((unsigned)n_wg);
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* b = static_cast<const uint8_t*>(blocks);
    const uint8_t* xp = static_cast<const uint8_t*>(x);
    uint16_t* yp = static_cast<uint16_t*>(y);
    dispatch_packed(q_type, [&](auto qt) {
        constexpr int QT = decltype(qt)::value;
        dispatch_bool(x_dtype == GQ_BF16, [&](auto bf16) {
            auto go = [&](auto w) {  // w: the 256-token tile
                hipLaunchKernelGGL((linear_packed_kernel<QT, decltype(bf16)::value, decltype(w)::value ? 256 : 128>), grid, dim3(256), 0,
                                   st, b, row_src, R, C, xp, T, yp, (uint32_t)n_rt);
            };
            if constexpr (wide_ok(QT)) dispatch_bool(wide, go);  // (no 256-token instance is built for the other types)
            else go(std::false_type{});
        });
    });
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
