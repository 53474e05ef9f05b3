// gq_q8_0.hip -- K20: the Q8_0 encoder (include/gptq_gguf_q8.h).  [R, C] fp32 / fp16 / bf16 -> block_q8_0 { fp16 d; int8 qs[32]; },
// ggml-quants.c quantize_row_q8_0_ref bit for bit; the host form is gguf_writer.quantize_q8_0 (numpy, six full-size fp32
// temporaries).
//
// HBM-bound streaming: 2 or 4 B/param read once, 34 / 32 = 1.0625 B/param written.  A workgroup of 256 threads takes a span
// of SPAN = 128 consecutive OUTPUT blocks per turn (output block L = r * C/32 + j encodes values 32 j .. 32 j + 31 of input
// row row_src[r]); thread (b, h) = (tid / 2, tid % 2) reads the 16 consecutive values of half h of block b with two (fp16 /
// bf16) or four (fp32) 16-byte loads -- rows are multiples of 32 values, so every such chunk is 32 / 64 bytes aligned when x
// is 16 --, widens them exactly, and takes the block's amax as max over its registers and one cross-lane exchange with lane
// tid ^ 1 (the two lanes of a block are neighbours in a wave; no LDS, no atomics).  Both lanes then compute the same d and
// id and their 16 codes.  A block is 34 bytes, 2-byte aligned: the codes are written to the span's image in LDS as 2-byte
// stores (4352 bytes = 272 x 16), and after a barrier the image goes out as 16-byte stores -- the span starts at byte
// b0 * 34 with b0 a multiple of 128, i.e. 16-byte aligned when `blocks` is.  The last span of a matrix may end on a
// partial 16-byte chunk: its tail (an even number of bytes) is written as 2-byte stores, nothing past R * C/32 * 34 is
// touched.  Every result depends on the block's 32 values only, never on the grid.
//
// Numerical contract (exact class; -ffp-contract=off, no fast-math, hipcc's correctly rounded fp32 division):
//   d = amax / 127.0f;  id = d != 0 ? 1.0f / d : 0;  q = roundf(x * id) (half away from zero);  d stored by f2h (RNE: may
//   round to 0 or overflow to inf).  |x * id| <= 127 (1 + 2^-22), so the int8 cast never wraps for finite input.
#include "../gq_common.hpp"
#include "../../../include/gptq_gguf_q8.h"

namespace gq {
namespace {

constexpr int SPAN = 128;               // blocks per turn: 256 threads x 16 values
constexpr int SPAN_BYTES = SPAN * 34;   // 4352 = 272 x 16

template <int SD> struct Src;
template <> struct Src<GQ_F32> { static constexpr int ES = 4; };
template <> struct Src<GQ_F16> { static constexpr int ES = 2; };
template <> struct Src<GQ_BF16> { static constexpr int ES = 2; };

// 16 consecutive values at p (16-byte aligned), widened exactly to fp32; all loads issued before the first use
template <int SD>
__device__ __forceinline__ void load16(const uint8_t* __restrict__ p, float v[16]) {
    constexpr int NQ = Src<SD>::ES;  // 16-byte loads: 16 values x ES bytes / 16
    uint4 w[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) w[q] = reinterpret_cast<const uint4*>(p)[q];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const uint32_t u[4] = {w[q].x, w[q].y, w[q].z, w[q].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (SD == GQ_F32) {
                v[4 * q + i] = __builtin_bit_cast(float, u[i]);
            } else if constexpr (SD == GQ_F16) {
                v[8 * q + 2 * i] = h2f((uint16_t)(u[i] & 0xffffu)), v[8 * q + 2 * i + 1] = h2f((uint16_t)(u[i] >> 16));
            } else {
                v[8 * q + 2 * i] = bf2f((uint16_t)(u[i] & 0xffffu)), v[8 * q + 2 * i + 1] = bf2f((uint16_t)(u[i] >> 16));
            }
        }
    }
}

template <int SD>
__global__ __launch_bounds__(256) void q8_0_encode_kernel(const uint8_t* __restrict__ x, const int32_t* __restrict__ row_src,
                                                          int64_t nblocks, uint32_t nbr, uint8_t* __restrict__ blocks) {
    constexpr int ES = Src<SD>::ES;
    __shared__ __attribute__((aligned(16))) uint8_t img[SPAN_BYTES];
    const int tid = threadIdx.x, b = tid >> 1, h = tid & 1;
    for (int64_t b0 = (int64_t)blockIdx.x * SPAN; b0 < nblocks; b0 += (int64_t)gridDim.x * SPAN) {
        const int nb = (int)((nblocks - b0) < SPAN ? (nblocks - b0) : SPAN);
        if (b < nb) {  // (both lanes of a block take the same side of this branch: the exchange below is between active lanes)
            // row and column block of output block b0 + b: one 64-bit division per workgroup (uniform), one 32-bit per thread
            const int64_t r0 = b0 / nbr;
            const uint32_t jl = (uint32_t)(b0 - r0 * nbr) + (uint32_t)b, dr = jl / nbr, j = jl - dr * nbr;
            const int64_t r = r0 + dr, sr = row_src ? (int64_t)row_src[r] : r;
            float v[16];
            load16<SD>(x + ((sr * nbr + j) * 32 + 16 * h) * ES, v);
            float amax = 0.0f;
#pragma unroll
            for (int k = 0; k < 16; ++k) amax = fmaxf(amax, fabsf(v[k]));
            amax = fmaxf(amax, __shfl_xor(amax, 1));
            const float d = amax / 127.0f;
            const float id = d != 0.0f ? 1.0f / d : 0.0f;
            uint16_t* ib = reinterpret_cast<uint16_t*>(img + b * 34);
            if (h == 0) ib[0] = f2h(d);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int q0 = (int)roundf(v[2 * k] * id), q1 = (int)roundf(v[2 * k + 1] * id);
                ib[1 + 8 * h + k] = (uint16_t)((uint32_t)(q0 & 0xff) | ((uint32_t)(q1 & 0xff) << 8));
            }
        }
        __syncthreads();
        const int nbytes = nb * 34, nfull = nbytes >> 4;
        uint8_t* ob = blocks + b0 * 34;
        for (int c = tid; c < nfull; c += 256) reinterpret_cast<uint4*>(ob)[c] = reinterpret_cast<const uint4*>(img)[c];
        const int t2 = (nfull << 3) + tid;  // the tail of the last span, in 2-byte units (at most 7 of them)
        if (t2 < (nbytes >> 1)) reinterpret_cast<uint16_t*>(ob)[t2] = reinterpret_cast<const uint16_t*>(img)[t2];
        __syncthreads();
    }
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_quantize_q8_0(const void* x, int x_dtype, int64_t R, int64_t C, const int32_t* row_src, uint8_t* blocks, void* stream) {
    if (int rc = options_ok()) return rc;
    if (x_dtype != GQ_F32 && x_dtype != GQ_F16 && x_dtype != GQ_BF16)
        GQ_FAIL(GQ_E_BAD_TYPE, "gq_quantize_q8_0: unknown x_dtype %d", x_dtype);
    if (R < 1 || C < 32 || C > 0x7fffffff || C % 32)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quantize_q8_0: R=%ld C=%ld (R >= 1, C %% 32 == 0, 32 <= C < 2^31)", (long)R, (long)C);
    if (!x || !blocks) GQ_FAIL(GQ_E_NULL, "gq_quantize_q8_0: null pointer");
    if (!aligned(x, 16) || !aligned(blocks, 16)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quantize_q8_0: x and blocks must be 16-byte aligned");
    if (!aligned(row_src, 4)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quantize_q8_0: row_src not 4-byte aligned");
    const uint32_t nbr = (uint32_t)(C / 32);
    if (R > INT64_MAX / 64 / nbr) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quantize_q8_0: R=%ld C=%ld is too large", (long)R, (long)C);
    const int64_t nblocks = R * nbr, spans = (nblocks + SPAN - 1) / SPAN;
    dim3 grid((unsigned)(spans < 16384 ? spans : 16384)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* xp = static_cast<const uint8_t*>(x);
    switch (x_dtype) {
    case GQ_F32: hipLaunchKernelGGL((q8_0_encode_kernel<GQ_F32>), grid, block, 0, st, xp, row_src, nblocks, nbr, blocks); break;
    case GQ_F16: hipLaunchKernelGGL((q8_0_encode_kernel<GQ_F16>), grid, block, 0, st, xp, row_src, nblocks, nbr, blocks); break;
    default: hipLaunchKernelGGL((q8_0_encode_kernel<GQ_BF16>), grid, block, 0, st, xp, row_src, nblocks, nbr, blocks); break;
    }
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
