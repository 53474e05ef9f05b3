// gq_iq4_encode.hip -- K27: the IQ4_NL / IQ4_XS encoder (include/gptq_gguf_iq4_encode.h).  [R, C] fp32 / fp16 / bf16, optionally with
// one importance value per column -> block_iq4_nl { fp16 d; uint8 qs[16]; } / block_iq4_xs { fp16 d; uint16 scales_h; uint8
// scales_l[4]; uint8 qs[128]; }.  The algorithm is the header's own contract (after the ntry = 7 path of ggml's
// quantize_row_iq4_nl_impl); the host form is gguf_writer.quantize_iq4 (numpy), byte for byte.
//
// Compute-bound, not HBM-bound: a block's scale is searched over 16 candidates, each a pass over its 32 values (a table search
// per value), and the contract fixes the order of every sum.  So ONE LANE OWNS ONE 32-VALUE BLOCK: its 32 values and 32 weights
// stay in registers through the 17 passes, and nothing is reduced across lanes but what the contract makes a super-block's:
// the 8 lanes of an IQ4_XS super-block are neighbours in a wave and exchange sigma2 (a chain of 8 steps, which keeps the sum in
// ascending j over all 256 values), the block scales (ms, D) and the 8 ls by cross-lane reads.  No atomics.
//
// A workgroup of 256 threads takes a tile of TILE = 256 consecutive OUTPUT blocks per turn (output block L = r * C/32 + j
// encodes values 32 j .. 32 j + 31 of input row row_src[r]; 256 blocks are 32 whole IQ4_XS super-blocks).  Each input byte is
// read once: the tile is staged through LDS with coalesced 16-byte loads -- a block's 64 / 128 bytes are contiguous and
// 16-byte aligned when x is -- at a pitch of 32 values + 16 bytes per block (36 / 20 dwords: an odd number of 16-byte
// units, so the 16 lanes of a ds_read_b128 group start on 16 different 4-bank groups of the 64 banks).  The output image
// of the tile (256 x 18 = 4608 or 32 x 136 = 4352 bytes, both multiples of 16) is built in LDS -- 2-byte stores for IQ4_NL's
// 2-byte aligned blocks, 8-byte stores for IQ4_XS -- and goes out as 16-byte stores: the tile starts at byte b0 * 18 or
// b0 * 17 with b0 a multiple of 256, 16-byte aligned when `blocks` is.  The last tile of a matrix may end on a partial
// 16-byte chunk: its tail (an even number of bytes) is written as 2-byte stores, nothing past the last block is touched.
// LDS: 36864 + 4608 + 68 bytes for fp32 input, three workgroups a CU.  The table lives in LDS (17 floats, kv and a
// sentinel): best() is a 4-step binary search over it, the lanes of a wave read at most 17 different addresses.
//
// Numerical contract (exact class; -ffp-contract=off, no fast-math, hipcc's correctly rounded fp32 division and sqrtf).
#include "../gq_common.hpp"
#include "../../../include/gptq_gguf_iq4_encode.h"
#include "gq_iq4_search.hpp"

namespace gq {
namespace {

constexpr int TILE = 256;  // 32-value blocks per turn: one lane each
constexpr int MAX_GRID = 4096;  // workgroups of a launch: beyond 4096 tiles (2^20 blocks) a workgroup takes further turns

template <int SD> struct Src;
template <> struct Src<GQ_F32> { static constexpr int ES = 4; };
template <> struct Src<GQ_F16> { static constexpr int ES = 2; };
template <> struct Src<GQ_BF16> { static constexpr int ES = 2; };

using namespace iq4;  // KV17, best and the candidate sums: gq_iq4_search.hpp, shared with the column walk on this grid

// 32 values of one block from its staged bytes at p (16-byte aligned), widened exactly to fp32
template <int SD>
__device__ __forceinline__ void load32(const uint8_t* p, float (&v)[32]) {
    constexpr int NQ = 2 * Src<SD>::ES;  // 16-byte reads
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const uint4 w = reinterpret_cast<const uint4*>(p)[k];
        const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (SD == GQ_F32) {
                v[4 * k + i] = __builtin_bit_cast(float, u[i]);
            } else if constexpr (SD == GQ_F16) {
                v[8 * k + 2 * i] = h2f((uint16_t)(u[i] & 0xffffu)), v[8 * k + 2 * i + 1] = h2f((uint16_t)(u[i] >> 16));
            } else {
                v[8 * k + 2 * i] = bf2f((uint16_t)(u[i] & 0xffffu)), v[8 * k + 2 * i + 1] = bf2f((uint16_t)(u[i] >> 16));
            }
        }
    }
}

// the 32 codes of a block under the inverse scale id: value j in the low nibble of byte j, value j + 16 in the high one
__device__ __forceinline__ void codes(const float* __restrict__ kvs, const float (&x)[32], float id, uint32_t (&qs)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t word = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int lo, hi;
            float q;
            best(kvs, id * x[4 * k + i], lo, q);
            best(kvs, id * x[4 * k + i + 16], hi, q);
            word |= (uint32_t)(lo | (hi << 4)) << (8 * i);
        }
        qs[k] = word;
    }
}

template <int SD, bool XS>
__global__ __launch_bounds__(256) void iq4_encode_kernel(const uint8_t* __restrict__ x, const float* __restrict__ importance,
                                                         const int32_t* __restrict__ row_src, int64_t nblocks, uint32_t nbr,
                                                         uint8_t* __restrict__ blocks) {
    constexpr int ES = Src<SD>::ES, PITCH = 32 * ES + 16, CPB = 2 * ES;  // bytes per staged block; 16-byte chunks per block
    constexpr int BB = XS ? 17 : 18;                                     // output bytes per 32-value block (136 / 8, 18)
    __shared__ __attribute__((aligned(16))) uint8_t tile[TILE * PITCH];
    __shared__ __attribute__((aligned(16))) uint8_t img[TILE * BB];
    __shared__ float kvs[17];
    const int tid = threadIdx.x;
    if (tid < 17) kvs[tid] = KV17[tid];  // (read after the first barrier below)
    for (int64_t b0 = (int64_t)blockIdx.x * TILE; b0 < nblocks; b0 += (int64_t)gridDim.x * TILE) {
        const int nb = (int)((nblocks - b0) < TILE ? (nblocks - b0) : TILE);
        // row and column block of output block b0 + b: one 64-bit division per workgroup (uniform), 32-bit ones per thread
        const int64_t r0 = b0 / nbr;
        const uint32_t j0 = (uint32_t)(b0 - r0 * nbr);
#pragma unroll
        for (int i = 0; i < CPB; ++i) {
            const int c = tid + 256 * i, b = c / CPB, k = c % CPB;
            if (b < nb) {
                const uint32_t jl = j0 + (uint32_t)b, dr = jl / nbr, j = jl - dr * nbr;
                const int64_t r = r0 + dr, sr = row_src ? (int64_t)row_src[r] : r;
                *reinterpret_cast<uint4*>(tile + b * PITCH + 16 * k) =
                    *reinterpret_cast<const uint4*>(x + ((sr * nbr + j) * 32) * ES + 16 * k);
            }
        }
        __syncthreads();
        if (tid < nb) {  // (IQ4_XS: nb is a multiple of 8, the 8 lanes of a super-block take the same side)
            float xv[32], w[32];
            load32<SD>(tile + tid * PITCH, xv);
            bool weighted = false;
            float sigma2 = 0.0f;
            if (importance) {  // (uniform)
                float s = 0.0f;
                if constexpr (XS) {  // ascending j over the 256 values: lane ib continues the sum of lane ib - 1
#pragma unroll 1
                    for (int ib = 0; ib < 8; ++ib) {
                        float t = s;
#pragma unroll
                        for (int j = 0; j < 32; ++j) t += xv[j] * xv[j];
                        s = __shfl(t, ib, 8);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 32; ++j) s += xv[j] * xv[j];
                }
                sigma2 = sigma2_of(s, XS ? 256.0f : 32.0f);
                const uint32_t jl = j0 + (uint32_t)tid, j = jl % nbr;
                const float4* ip = reinterpret_cast<const float4*>(importance + (size_t)j * 32);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float4 v = ip[k];
                    w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
                }
#pragma unroll
                for (int j2 = 0; j2 < 32; ++j2) weighted = weighted || w[j2] != 0.0f;
            } else {
#pragma unroll
                for (int j = 0; j < 32; ++j) w[j] = 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 32; ++j) w[j] = weight_of(xv[j], w[j], sigma2, weighted);  // (not weighted: none, or all zero here)
            float amax, mx;
            block_max(xv, amax, mx);
            float d = 0.0f;
            if (!(amax < 1e-15f)) {
                float bst = 0.0f;
#pragma unroll 1
                for (int itry = -8; itry <= 7; ++itry) {
                    float sumqx, sumq2;
                    cand_sums(kvs, xv, w, cand_id(itry, mx), sumqx, sumq2);
                    cand_take(itry, sumqx, sumq2, d, bst);
                }
            }
            uint32_t qs[4];
            if constexpr (!XS) {
                codes(kvs, xv, nl_inverse(d), qs);
                uint16_t* ob = reinterpret_cast<uint16_t*>(img + tid * 18);
                ob[0] = f2h(d);
#pragma unroll
                for (int k = 0; k < 4; ++k) ob[1 + 2 * k] = (uint16_t)(qs[k] & 0xffffu), ob[2 + 2 * k] = (uint16_t)(qs[k] >> 16);
            } else {
                float dmax = 0.0f, ms = 0.0f;  // the block scale of largest |d|, the first one on a tie
                for (int ib = 0; ib < 8; ++ib) {
                    const float v = __shfl(d, ib, 8);
                    if (fabsf(v) > dmax) dmax = fabsf(v), ms = v;
                }
                const float D = xs_super_scale(ms);
                float lf, dl, idl;
                xs_block_scale(D, d, lf, dl, idl);
                codes(kvs, xv, idl, qs);
                const uint32_t ls = (uint32_t)((int)lf + 32);
                uint32_t scales_h = 0, scales_l = 0;
                for (int ib = 0; ib < 8; ++ib) {
                    const uint32_t v = (uint32_t)__shfl((int)ls, ib, 8);
                    scales_h |= (v >> 4) << (2 * ib);
                    scales_l |= (v & 15u) << (4 * ib);  // byte ib / 2, nibble ib % 2
                }
                uint8_t* sb = img + (tid >> 3) * 136;
                if ((tid & 7) == 0) *reinterpret_cast<uint2*>(sb) = make_uint2((uint32_t)f2h(D) | (scales_h << 16), scales_l);
                uint2* ob = reinterpret_cast<uint2*>(sb + 8 + 16 * (tid & 7));
                ob[0] = make_uint2(qs[0], qs[1]);
                ob[1] = make_uint2(qs[2], qs[3]);
            }
        }
        __syncthreads();
        const int nbytes = nb * BB, nfull = nbytes >> 4;
        uint8_t* ob = blocks + b0 * BB;
        for (int c = tid; c < nfull; c += 256) reinterpret_cast<uint4*>(ob)[c] = reinterpret_cast<const uint4*>(img)[c];
        const int t2 = (nfull << 3) + tid;  // the tail of the last tile, in 2-byte units (at most 7 of them)
        if (t2 < (nbytes >> 1)) reinterpret_cast<uint16_t*>(ob)[t2] = reinterpret_cast<const uint16_t*>(img)[t2];
        // (no third barrier: the next turn writes `tile` only before its first barrier, `img` only after it)
    }
}

template <int SD>
void launch(bool xs, dim3 grid, hipStream_t st, const uint8_t* x, const float* importance, const int32_t* row_src, int64_t nblocks,
            uint32_t nbr, uint8_t* blocks) {
    if (xs)
        hipLaunchKernelGGL((iq4_encode_kernel<SD, true>), grid, dim3(256), 0, st, x, importance, row_src, nblocks, nbr, blocks);
    else
        hipLaunchKernelGGL((iq4_encode_kernel<SD, false>), grid, dim3(256), 0, st, x, importance, row_src, nblocks, nbr, blocks);
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_quantize_iq4(const void* x, int x_dtype, int64_t R, int64_t C, int q_type, const float* importance, const int32_t* row_src,
                    uint8_t* blocks, void* stream) {
    if (int rc = options_ok()) return rc;
    if (x_dtype != GQ_F32 && x_dtype != GQ_F16 && x_dtype != GQ_BF16)
        GQ_FAIL(GQ_E_BAD_TYPE, "gq_quantize_iq4: unknown x_dtype %d", x_dtype);
    if (q_type != GQ_IQ4_NL && q_type != GQ_IQ4_XS)
        GQ_FAIL(GQ_E_BAD_TYPE, "gq_quantize_iq4: q_type %d is neither GQ_IQ4_NL (20) nor GQ_IQ4_XS (23)", q_type);
    const bool xs = q_type == GQ_IQ4_XS;
    if (R < 1 || C < 32 || C > 0x7fffffff || C % (xs ? 256 : 32))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quantize_iq4: R=%ld C=%ld (R >= 1, C %% %d == 0, 32 <= C < 2^31)", (long)R, (long)C, xs ? 256 : 32);
    if (!x || !blocks) GQ_FAIL(GQ_E_NULL, "gq_quantize_iq4: null pointer");
    if (!aligned(x, 16) || !aligned(blocks, 16)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quantize_iq4: x and blocks must be 16-byte aligned");
    if (!aligned(importance, 16)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quantize_iq4: importance not 16-byte aligned");
    if (!aligned(row_src, 4)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quantize_iq4: row_src not 4-byte aligned");
    const uint32_t nbr = (uint32_t)(C / 32);
    if (R > INT64_MAX / 64 / nbr) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_quantize_iq4: R=%ld C=%ld is too large", (long)R, (long)C);
    const int64_t nblocks = R * nbr, tiles = (nblocks + TILE - 1) / TILE;
    dim3 grid((unsigned)(tiles < MAX_GRID ? tiles : MAX_GRID));
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* xp = static_cast<const uint8_t*>(x);
    switch (x_dtype) {
    case GQ_F32: launch<GQ_F32>(xs, grid, st, xp, importance, row_src, nblocks, nbr, blocks); break;
    case GQ_F16: launch<GQ_F16>(xs, grid, st, xp, importance, row_src, nblocks, nbr, blocks); break;
    default: launch<GQ_BF16>(xs, grid, st, xp, importance, row_src, nblocks, nbr, blocks); break;
    }
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
