// gq_moe_gemv.hip -- K24: the grouped expert GEMV of a packed MoE layer's decode step.  One launch multiplies every
// (token, expert) pair of the step with its expert's weight, read as the GGUF block bytes of the stacked [E, R, C] tensor:
// y[p] = W[pair_expert[p]] x[p / pairs_per_row].  The expert ids stay on the device; nothing is read back, sorted or counted
// on the host.
//
// Form: K22's (gq_qgemv.hip), with a second grid dimension.  Workgroup (b, e) owns rows 16 b .. 16 b + 15 of expert e and all
// of C, with min(16, C / 256) waves.  Every wave first reads the P <= 64 expert ids, one per lane, and forms the mask of the
// pairs that name e with a ballot; the mask is the same in every wave, so no LDS and no barrier is spent on it.  A workgroup
// whose expert no pair names returns there, before any staging: the weight bytes of an expert that is not hit are never
// read.  Otherwise MFMA column i carries the i-th matching pair in pair order: its input row and its output row replace
// K22's token t.  More than 16 matching pairs take further passes of 16 with the weight staged again (a decode step with
// distinct experts per token and T <= 16 never has them; nothing relies on that).
// The K loop, the wave-order reduction and the store are gq_gemv_core.hpp's gemv_pass, the text gq_gemv_packed runs: an MFMA
// column depends on its own B column only, so row p of y is bit for bit gq_gemv_packed's result for that expert's slice and
// that input row at T = 1.  No atomics, no workspace, no scratch, no host synchronisation.
#include "../../../include/gptq_gguf_moe.h"

#include "gq_gemv_core.hpp"

namespace gq {
namespace {

using namespace gemvcore;

// the position of the n-th (from 0) set bit of m, n < popcount(m): six halvings, no cross-lane traffic
__device__ __forceinline__ int nth_set_bit(uint64_t m, int n) {
    int pos = 0;
#pragma unroll
    for (int w = 32; w; w >>= 1) {
        const int c = __builtin_popcountll((m >> pos) & ((1ull << w) - 1));
        if (n >= c) n -= c, pos += w;
    }
    return pos;
}

template <int QT, bool BF16>
__global__ __launch_bounds__(64 * MAX_NW) void gemv_packed_experts_kernel(const uint8_t* __restrict__ blocks, int64_t R, int64_t C,
                                                                          const uint8_t* __restrict__ x,
                                                                          const int32_t* __restrict__ pair_expert, int P,
                                                                          int pairs_per_row, uint16_t* __restrict__ y) {
    using Q = QL<QT>;
    __shared__ __attribute__((aligned(16))) uint8_t smem[smem_bytes<QT>()];
    const int lane = threadIdx.x & 63, e = blockIdx.y;
    // bit p: pair p names this workgroup's expert (ids outside [0, E) match no workgroup: such a pair is skipped)
    const uint64_t m = __ballot(lane < P && pair_expert[lane] == e);
    if (m == 0) return;  // uniform over the workgroup: every wave read the same ids
    const int64_t r0 = (int64_t)blockIdx.x * VR, nsb = C / 256;
    const int nr = (int)((R - r0) < VR ? (R - r0) : VR);
    const int nm = __builtin_popcountll(m);
    for (int first = 0;;) {  // a pass: the matching pairs first .. first + 15, one per MFMA column
        // the thread index is made opaque per pass: what a pass derives from it is then derived again by the next pass instead of
        // staying in registers through the epilogue (with it Q3_K needs more than the 128 VGPRs of a 16-wave workgroup)
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int l15 = tid & 15, n = first + l15;
        const int64_t base = l15 < nr ? ((int64_t)e * R + r0 + l15) * nsb * Q::ROWB : 0;  // row l15 of expert e: its first block
        const int p = n < nm ? nth_set_bit(m, n) : 0;
        gemv_pass<QT, BF16>(tid, blocks, base, nr, r0, R, C, n < nm, x, p / pairs_per_row, y,
                            [=] {  // the pair again, from the mask: one register less through the K loop
                                int t = threadIdx.x;
                                asm volatile("" : "+v"(t));
                                return nth_set_bit(m, first + (t & 15));
                            },
                            smem);
        if ((first += VR) >= nm) return;
        __syncthreads();  // wave 0 has read every wave's partial sums: the slots may be staged again
    }
}

template <int QT>
void launch(bool bf16, dim3 grid, int nw, hipStream_t st, const uint8_t* blocks, int64_t R, int64_t C, const uint8_t* x,
            const int32_t* pe, int P, int ppr, uint16_t* y) {
    if (bf16) hipLaunchKernelGGL((gemv_packed_experts_kernel<QT, true>), grid, dim3(64 * nw), 0, st, blocks, R, C, x, pe, P, ppr, y);
    else hipLaunchKernelGGL((gemv_packed_experts_kernel<QT, false>), grid, dim3(64 * nw), 0, st, blocks, R, C, x, pe, P, ppr, y);
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_gemv_packed_experts(int q_type, const void* blocks, int64_t E, int64_t R, int64_t C, const void* x, int64_t x_rows,
                           const int32_t* pair_expert, int64_t P, int64_t pairs_per_row, int x_dtype, void* y, void* stream) {
    if (int rc = options_ok()) return rc;
    if (!packed_type(q_type))
        GQ_FAIL(GQ_E_BAD_TYPE, "gq_gemv_packed_experts: unknown q_type %d (a K-quant, GQ_Q8_0, GQ_IQ4_NL or GQ_IQ4_XS)", q_type);
    if (x_dtype != GQ_F16 && x_dtype != GQ_BF16)
        GQ_FAIL(GQ_E_BAD_TYPE, "gq_gemv_packed_experts: x_dtype %d (GQ_F16 or GQ_BF16; there is no fp32 path)", x_dtype);
    if (!blocks) GQ_FAIL(GQ_E_NULL, "gq_gemv_packed_experts: blocks is NULL");
    if (!x) GQ_FAIL(GQ_E_NULL, "gq_gemv_packed_experts: x is NULL");
    if (!pair_expert) GQ_FAIL(GQ_E_NULL, "gq_gemv_packed_experts: pair_expert is NULL");
    if (!y) GQ_FAIL(GQ_E_NULL, "gq_gemv_packed_experts: y is NULL");
    if (E < 1 || E > 65535) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed_experts: E=%ld (not in [1, 65535])", (long)E);
    if (R < 1 || R > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed_experts: R=%ld (not in [1, 2^31))", (long)R);
    if (P < 1 || P > GQ_MOE_MAX_PAIRS)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed_experts: P=%ld (not in [1, %d] pairs)", (long)P, GQ_MOE_MAX_PAIRS);
    if (pairs_per_row < 1 || x_rows < 1 || pairs_per_row > P || x_rows > P || x_rows * pairs_per_row != P)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed_experts: x_rows=%ld * pairs_per_row=%ld != P=%ld", (long)x_rows,
                (long)pairs_per_row, (long)P);
    if (C < 256 || C > 0x7fffffff || C % 256)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed_experts: C=%ld (C %% 256 != 0 or not in [256, 2^31); Q8_0 and IQ4_NL included)", (long)C);
    const int al = block_align(q_type);
    if (!aligned(blocks, al)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed_experts: blocks not %d-byte aligned", al);
    if (!aligned(pair_expert, 4)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed_experts: pair_expert not 4-byte aligned");
    if (!aligned(x, 16)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed_experts: x not 16-byte aligned");
    if (!aligned(y, 16)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed_experts: y not 16-byte aligned");
    const int64_t nsb = C / 256;
    const int nw = (int)(nsb < MAX_NW ? nsb : MAX_NW);
    const dim3 grid((unsigned)((R + VR - 1) / VR), (unsigned)E);  // x < 2^27, y <= 65535
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* b = static_cast<const uint8_t*>(blocks);
    const uint8_t* xp = static_cast<const uint8_t*>(x);
    uint16_t* yp = static_cast<uint16_t*>(y);
    const bool bf = x_dtype == GQ_BF16;
    const int np = (int)P, ppr = (int)pairs_per_row;
    switch (q_type) {
    case GQ_Q2_K: launch<GQ_Q2_K>(bf, grid, nw, st, b, R, C, xp, pair_expert, np, ppr, yp); break;
    case GQ_Q3_K: launch<GQ_Q3_K>(bf, grid, nw, st, b, R, C, xp, pair_expert, np, ppr, yp); break;
    case GQ_Q4_K: launch<GQ_Q4_K>(bf, grid, nw, st, b, R, C, xp, pair_expert, np, ppr, yp); break;
    case GQ_Q5_K: launch<GQ_Q5_K>(bf, grid, nw, st, b, R, C, xp, pair_expert, np, ppr, yp); break;
    case GQ_Q6_K: launch<GQ_Q6_K>(bf, grid, nw, st, b, R, C, xp, pair_expert, np, ppr, yp); break;
    case GQ_IQ4_NL: launch<GQ_IQ4_NL>(bf, grid, nw, st, b, R, C, xp, pair_expert, np, ppr, yp); break;
    case GQ_IQ4_XS: launch<GQ_IQ4_XS>(bf, grid, nw, st, b, R, C, xp, pair_expert, np, ppr, yp); break;
    default: launch<GQ_Q8_0>(bf, grid, nw, st, b, R, C, xp, pair_expert, np, ppr, yp); break;
    }
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
