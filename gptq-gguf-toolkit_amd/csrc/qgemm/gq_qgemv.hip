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

#include "../search/gq_block_host.hpp"
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

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_gemv_packed(int q_type, const void* blocks, const int32_t* row_src, int64_t R, int64_t C, const void* x, int64_t T,
                   int x_dtype, void* y, void* stream) {
    if (int rc = options_ok()) return rc;
    const char* who = "gq_gemv_packed";
    if (int rc = check_types(who, q_type, x_dtype)) return rc;
    if (int rc = need(who, "blocks", blocks)) return rc;
    if (int rc = need(who, "x", x)) return rc;
    if (int rc = need(who, "y", y)) return rc;
    if (int rc = check_R(who, R)) return rc;
    if (T < 1 || T > GQ_GEMV_MAX_T)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed: T=%ld (not in [1, %d]; gq_linear_packed takes more tokens)", (long)T, GQ_GEMV_MAX_T);
    if (int rc = check_C256(who, C)) return rc;
    if (int rc = check_blocks_aligned(who, q_type, blocks)) return rc;
    if (int rc = check_aligned(who, "row_src", row_src, 4)) return rc;
    if (int rc = check_aligned(who, "x", x, 16)) return rc;
    if (int rc = check_aligned(who, "y", y, 16)) return rc;
    const int64_t nsb = C / 256;
    const int nw = (int)(nsb < MAX_NW ? nsb : MAX_NW);
    const dim3 grid((unsigned)((R + VR - 1) / VR));  // < 2^27
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* b = static_cast<const uint8_t*>(blocks);
    const uint8_t* xp = static_cast<const uint8_t*>(x);
    uint16_t* yp = static_cast<uint16_t*>(y);
    dispatch_packed(q_type, [&](auto qt) {
        dispatch_bool(x_dtype == GQ_BF16, [&](auto bf16) {
            hipLaunchKernelGGL((gemv_packed_kernel<decltype(qt)::value, decltype(bf16)::value>), grid, dim3(64 * nw), 0, st, b, row_src, R,
                               C, xp, (int)T, yp);
        });
    });
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
