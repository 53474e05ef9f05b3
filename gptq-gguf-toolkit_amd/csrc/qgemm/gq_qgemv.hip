// gq_qgemv.hip -- K22: y = x W^T for 1 <= T <= 16 tokens and a weight [R, C] that exists only as GGUF block bytes (K-quants,
// Q8_0, IQ4_NL, IQ4_XS): the decode step of a packed model.  gq_gemv_packed has the contract of gq_linear_packed (K21) -- the same operand
// bits, fp32 accumulation, one rounding -- at the shape where that kernel launches R / 128 workgroups and fills 127 of 128
// tokens of its tile with zeros.  Here the call is one stream over the weight bytes, spread over the whole device.
//
// Form: v_mfma_f32_16x16x32_{f16,bf16} with A = 16 rows of W and B = the (at most 16) tokens, fragments as in K21: lane l
// holds W[r = l & 15][8 (l >> 4) + j] and x[t = l & 15][8 (l >> 4) + j], D[r = 4 (l >> 4) + i][t = l & 15] in register i.  The
// matrix pipe does the T-fold work, so one kernel serves every T and the cost per weight is the decode alone.
//
// A workgroup owns 16 rows and all of C; its NW = min(16, C / 256) waves take the superblocks j = w, w + NW, ... of those
// rows (K split across the waves of ONE workgroup, never across workgroups).  A [4096, 4096] weight is 256 workgroups of 16
// waves, one superblock of 16 rows each.  Per superblock a wave
//   * loads its x fragment straight to registers: lane (t, q) reads x[t][256 j + 64 c + 16 q .. + 15] for c = 0 .. 3, two
//     16-byte loads per chunk, chunk c + 1's in flight during chunk c's decode (lanes with t >= T load nothing and hold
//     zeros); x is re-read by every workgroup and comes from the caches;
//   * stages the 16 rows' packed bytes of the superblock in its own LDS slots with loads of the type's natural alignment that
//     cover exactly the blocks' bytes (QL<QT>, the slot layout of K21), consecutive lanes on consecutive bytes of a row;
//   * decodes per 64-k chunk the 16 consecutive values of its row with decode16 (block_d / group_scale / codes16 / dequantize1
//     / cvt_out: the operand bits are gq_dequantize_blocks') and issues two MFMAs.
// The LDS slots are wave-private: a wavefront-scope fence orders the staging writes and the decode reads, no workgroup barrier
// sits in the K loop.  The staging goes through LDS for every type, Q4_K and Q5_K included: the A fragment of an MFMA is 16
// different rows per instruction, so direct loads would be 16-byte pieces 16 rows apart; staged, a row's bytes are read once,
// contiguously.
// The partial sums of the NW waves meet in LDS (each wave's 1 KB at the start of its own slots) after the one barrier of the
// kernel; wave 0 adds them in wave order 0, 1, .. NW - 1 and stores: deterministic, no atomics, no workspace.
// Rows >= R of the last workgroup are not staged (their slots hold stale bytes; an MFMA row depends on its own A row only, and
// those D rows are never stored).  y is stored 8 bytes wide where R % 4 == 0, else 2 bytes wide with a row check.
#include "../../../include/gptq_gguf_qgemv.h"

#include "gq_gemv_core.hpp"  // the K loop, the reduction and the store: one text with gq_moe_gemv.hip (K24)

namespace gq {
namespace {

using namespace gemvcore;

template <int QT, bool BF16>
__global__ __launch_bounds__(64 * MAX_NW) void gemv_packed_kernel(const uint8_t* __restrict__ blocks,
                                                                  const int32_t* __restrict__ row_src, int64_t R, int64_t C,
                                                                  const uint8_t* __restrict__ x, int T, uint16_t* __restrict__ y) {
    using Q = QL<QT>;
    __shared__ __attribute__((aligned(16))) uint8_t smem[smem_bytes<QT>()];
    const int l15 = threadIdx.x & 15;
    const int64_t r0 = (int64_t)blockIdx.x * VR, nsb = C / 256;
    const int nr = (int)((R - r0) < VR ? (R - r0) : VR);
    const int64_t base = l15 < nr ? (row_src ? (int64_t)row_src[r0 + l15] : r0 + l15) * nsb * Q::ROWB : 0;  // row l15's first block
    // MFMA column l15 is token l15 (read only where l15 < T)
    gemv_pass<QT, BF16>(threadIdx.x, blocks, base, nr, r0, R, C, l15 < T, x, l15, y, [=] { return l15; }, smem);
}

template <int QT>
void launch(bool bf16, dim3 grid, int nw, hipStream_t st, const uint8_t* blocks, const int32_t* row_src, int64_t R, int64_t C,
            const uint8_t* x, int T, uint16_t* y) {
    if (bf16) hipLaunchKernelGGL((gemv_packed_kernel<QT, true>), grid, dim3(64 * nw), 0, st, blocks, row_src, R, C, x, T, y);
    else hipLaunchKernelGGL((gemv_packed_kernel<QT, false>), grid, dim3(64 * nw), 0, st, blocks, row_src, R, C, x, T, y);
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_gemv_packed(int q_type, const void* blocks, const int32_t* row_src, int64_t R, int64_t C, const void* x, int64_t T,
                   int x_dtype, void* y, void* stream) {
    if (int rc = options_ok()) return rc;
    if (!packed_type(q_type))
        GQ_FAIL(GQ_E_BAD_TYPE, "gq_gemv_packed: unknown q_type %d (a K-quant, GQ_Q8_0, GQ_IQ4_NL or GQ_IQ4_XS)", q_type);
    if (x_dtype != GQ_F16 && x_dtype != GQ_BF16)
        GQ_FAIL(GQ_E_BAD_TYPE, "gq_gemv_packed: x_dtype %d (GQ_F16 or GQ_BF16; there is no fp32 path)", x_dtype);
    if (!blocks) GQ_FAIL(GQ_E_NULL, "gq_gemv_packed: blocks is NULL");
    if (!x) GQ_FAIL(GQ_E_NULL, "gq_gemv_packed: x is NULL");
    if (!y) GQ_FAIL(GQ_E_NULL, "gq_gemv_packed: y is NULL");
    if (R < 1 || R > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed: R=%ld (not in [1, 2^31))", (long)R);
    if (T < 1 || T > GQ_GEMV_MAX_T)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed: T=%ld (not in [1, %d]; gq_linear_packed takes more tokens)", (long)T, GQ_GEMV_MAX_T);
    if (C < 256 || C > 0x7fffffff || C % 256)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed: C=%ld (C %% 256 != 0 or not in [256, 2^31); Q8_0 and IQ4_NL included)", (long)C);
    const int al = block_align(q_type);
    if (!aligned(blocks, al)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed: blocks not %d-byte aligned", al);
    if (!aligned(row_src, 4)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed: row_src not 4-byte aligned");
    if (!aligned(x, 16)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed: x not 16-byte aligned");
    if (!aligned(y, 16)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed: y not 16-byte aligned");
    const int64_t nsb = C / 256;
    const int nw = (int)(nsb < MAX_NW ? nsb : MAX_NW);
    const dim3 grid((unsigned)((R + VR - 1) / VR));  // < 2^27
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* b = static_cast<const uint8_t*>(blocks);
    const uint8_t* xp = static_cast<const uint8_t*>(x);
    uint16_t* yp = static_cast<uint16_t*>(y);
    const bool bf = x_dtype == GQ_BF16;
    switch (q_type) {
    case GQ_Q2_K: launch<GQ_Q2_K>(bf, grid, nw, st, b, row_src, R, C, xp, (int)T, yp); break;
    case GQ_Q3_K: launch<GQ_Q3_K>(bf, grid, nw, st, b, row_src, R, C, xp, (int)T, yp); break;
    case GQ_Q4_K: launch<GQ_Q4_K>(bf, grid, nw, st, b, row_src, R, C, xp, (int)T, yp); break;
    case GQ_Q5_K: launch<GQ_Q5_K>(bf, grid, nw, st, b, row_src, R, C, xp, (int)T, yp); break;
    case GQ_Q6_K: launch<GQ_Q6_K>(bf, grid, nw, st, b, row_src, R, C, xp, (int)T, yp); break;
    case GQ_IQ4_NL: launch<GQ_IQ4_NL>(bf, grid, nw, st, b, row_src, R, C, xp, (int)T, yp); break;
    case GQ_IQ4_XS: launch<GQ_IQ4_XS>(bf, grid, nw, st, b, row_src, R, C, xp, (int)T, yp); break;
    default: launch<GQ_Q8_0>(bf, grid, nw, st, b, row_src, R, C, xp, (int)T, yp); break;
    }
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
