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

#include "../search/gq_block_host.hpp"
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

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_gemv_packed_experts(int q_type, const void* blocks, int64_t E, int64_t R, int64_t C, const void* x, int64_t x_rows,
                           const int32_t* pair_expert, int64_t P, int64_t pairs_per_row, int x_dtype, void* y, void* stream) {
    if (int rc = options_ok()) return rc;
    const char* who = "gq_gemv_packed_experts";
    if (int rc = check_types(who, q_type, x_dtype)) return rc;
    if (int rc = need(who, "blocks", blocks)) return rc;
    if (int rc = need(who, "x", x)) return rc;
    if (int rc = need(who, "pair_expert", pair_expert)) return rc;
    if (int rc = need(who, "y", y)) return rc;
    if (E < 1 || E > 65535) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed_experts: E=%ld (not in [1, 65535])", (long)E);
    if (int rc = check_R(who, R)) return rc;
    if (P < 1 || P > GQ_MOE_MAX_PAIRS)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gemv_packed_experts: P=%ld (not in [1, %d] pairs)", (long)P, GQ_MOE_MAX_PAIRS);
    if (int rc = check_pairs(who, x_rows, pairs_per_row, P)) return rc;
    if (int rc = check_C256(who, C)) return rc;
    if (int rc = check_blocks_aligned(who, q_type, blocks)) return rc;
    if (int rc = check_aligned(who, "pair_expert", pair_expert, 4)) return rc;
    if (int rc = check_aligned(who, "x", x, 16)) return rc;
    if (int rc = check_aligned(who, "y", y, 16)) return rc;
    const int64_t nsb = C / 256;
    const int nw = (int)(nsb < MAX_NW ? nsb : MAX_NW);
    const dim3 grid((unsigned)((R + VR - 1) / VR), (unsigned)E);  // x < 2^27, y <= 65535
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* b = static_cast<const uint8_t*>(blocks);
    const uint8_t* xp = static_cast<const uint8_t*>(x);
    uint16_t* yp = static_cast<uint16_t*>(y);
    dispatch_packed(q_type, [&](auto qt) {
        dispatch_bool(x_dtype == GQ_BF16, [&](auto bf16) {
            hipLaunchKernelGGL((gemv_packed_experts_kernel<decltype(qt)::value, decltype(bf16)::value>), grid, dim3(64 * nw), 0, st, b, R,
                               C, xp, pair_expert, (int)P, (int)pairs_per_row, yp);
        });
    });
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
