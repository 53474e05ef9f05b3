// gq_iq4_gptq.hip -- K28: what the column walk on the IQ4_XS / IQ4_NL grid (include/gptq_gguf_iq4_gptq.h; the walk itself is
// gq_gptq.hip's, WalkKind::Iq4) needs besides its segment kernel: the lazy scale step of a 256-column group and the packer of
// the walk's outputs.
//
// The lazy scale step sits on the walk's critical path once per 256 columns, on the fp32 panel [R, 256] at row stride C.  One
// lane per 32-value block, the encoder's mapping, would leave the chip at two waves a CU for R = 4096; the 16 candidates of a
// block are independent of one another and only the selection is sequential.  So ONE LANE OWNS ONE CANDIDATE: 16 neighbouring
// lanes share a block, each runs the header's pass over the 32 values for its own inverse scale (gq_iq4_search.hpp, the
// encoder's text), and the header's selection then runs over the 16 (sumqx, sumq2) pairs in its order, in every lane of the
// group alike -- the same operations on the same values as the encoder's loop.  A workgroup of 256 threads takes two rows
// (2 x 8 blocks x 16 candidates); the rows, the weights and the block scales go through LDS.
#include "../gq_common.hpp"
#include "../gq_walk.hpp"
#include "../../../include/gptq_gguf_iq4_gptq.h"
#include "gq_iq4_search.hpp"

namespace gq {
namespace {

using namespace iq4;

constexpr int SS_ROWS = 2;  // rows of a workgroup of the scale step

// x: the panel, already at column a (16-byte aligned, ld % 4 == 0); imp: importance + a or nullptr; d / ls / step / istep:
// already at the group's first block; d_ld: row stride of d (C / 256 for XS, C / 32 for NL), nbr = C / 32: that of the rest.
template <bool XS>
__global__ __launch_bounds__(256) void iq4_scale_step_kernel(const float* __restrict__ x, int64_t R, int64_t ld,
                                                             const float* __restrict__ imp, uint16_t* __restrict__ d, int64_t d_ld,
                                                             uint8_t* __restrict__ ls, float* __restrict__ step,
                                                             float* __restrict__ istep, int64_t nbr) {
    __shared__ __attribute__((aligned(16))) float xs[SS_ROWS][256];
    __shared__ __attribute__((aligned(16))) float ws[SS_ROWS][256];
    __shared__ __attribute__((aligned(16))) float ims[256];
    __shared__ float sig[SS_ROWS][8], dsh[SS_ROWS][8];
    __shared__ float kvs[17];
    const int tid = threadIdx.x, rl = tid >> 7, ib = (tid >> 4) & 7, c = tid & 15;
    const int64_t row = (int64_t)blockIdx.x * SS_ROWS + rl;
    if (tid < 17) kvs[tid] = KV17[tid];
    if (tid < SS_ROWS * 64) {  // a row is 64 float4; a row past R reads as zeros and writes nothing
        const int64_t r = (int64_t)blockIdx.x * SS_ROWS + (tid >> 6);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < R) v = *reinterpret_cast<const float4*>(x + r * ld + (tid & 63) * 4);
        *reinterpret_cast<float4*>(&xs[tid >> 6][(tid & 63) * 4]) = v;
    } else if (imp && tid < SS_ROWS * 64 + 64) {
        *reinterpret_cast<float4*>(&ims[(tid & 63) * 4]) = *reinterpret_cast<const float4*>(imp + (tid & 63) * 4);
    }
    __syncthreads();
    if (imp) {  // (uniform) sigma2: the sum of squares in ascending j, one lane per super-block
        if (c == 0 && (XS ? ib == 0 : true)) {
            const float* xp = XS ? xs[rl] : xs[rl] + 32 * ib;
            float s = 0.0f;
            for (int j = 0; j < (XS ? 256 : 32); ++j) s += xp[j] * xp[j];
            sig[rl][XS ? 0 : ib] = sigma2_of(s, XS ? 256.0f : 32.0f);
        }
        __syncthreads();
    }
    float xv[32], w[32];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(&xs[rl][32 * ib + 4 * k]);
        xv[4 * k] = v.x, xv[4 * k + 1] = v.y, xv[4 * k + 2] = v.z, xv[4 * k + 3] = v.w;
    }
    {  // the weights of the block: lane c makes those of values 2c and 2c + 1
        bool weighted = false;
        float sigma2 = 0.0f, i0 = 0.0f, i1 = 0.0f;
        if (imp) {
            for (int j = 0; j < 32; ++j) weighted = weighted || ims[32 * ib + j] != 0.0f;
            sigma2 = sig[rl][XS ? 0 : ib];
            i0 = ims[32 * ib + 2 * c], i1 = ims[32 * ib + 2 * c + 1];
        }
        ws[rl][32 * ib + 2 * c] = weight_of(xs[rl][32 * ib + 2 * c], i0, sigma2, weighted);
        ws[rl][32 * ib + 2 * c + 1] = weight_of(xs[rl][32 * ib + 2 * c + 1], i1, sigma2, weighted);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(&ws[rl][32 * ib + 4 * k]);
        w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
    }
    float amax, mx;
    block_max(xv, amax, mx);
    const bool searched = !(amax < 1e-15f);  // (the same in the 16 lanes of a block)
    float sumqx = 0.0f, sumq2 = 0.0f;
    if (searched) cand_sums(kvs, xv, w, cand_id(c - 8, mx), sumqx, sumq2);
    float dblk = 0.0f, bst = 0.0f;
    for (int k = 0; k < 16; ++k) {  // the header's selection in its order itry = -8 .. 7, in every lane of the group
        const float sx = __shfl(sumqx, k, 16), s2 = __shfl(sumq2, k, 16);
        if (searched) cand_take(k - 8, sx, s2, dblk, bst);
    }
    if (c == 0) dsh[rl][ib] = dblk;
    __syncthreads();
    if (c != 0 || row >= R) return;
    if constexpr (XS) {
        float dmax = 0.0f, ms = 0.0f;  // the block scale of largest |d|, the first one on a tie
        for (int k = 0; k < 8; ++k) {
            const float v = dsh[rl][k];
            if (fabsf(v) > dmax) dmax = fabsf(v), ms = v;
        }
        const float D = xs_super_scale(ms);
        float lf, dl, idl;
        xs_block_scale(D, dblk, lf, dl, idl);
        const uint16_t Dh = f2h(D);
        if (ib == 0) d[row * d_ld] = Dh;
        const int l = (int)lf;
        ls[row * nbr + ib] = (uint8_t)(l + 32);
        step[row * nbr + ib] = h2f(Dh) * (float)l;  // the decoder's (ls - 32), an integer: lf may be -0
        istep[row * nbr + ib] = idl;
    } else {
        const uint16_t dh = f2h(dblk);
        d[row * d_ld + ib] = dh;
        step[row * nbr + ib] = h2f(dh);
        istep[row * nbr + ib] = nl_inverse(dblk);
    }
}

// ---- the packer.  A workgroup of 256 threads takes 256 consecutive OUTPUT blocks of 32 values per turn (32 whole IQ4_XS
// super-blocks), one thread each; the tile's image (256 x 18 = 4608 or 32 x 136 = 4352 bytes, both multiples of 16) is built
// in LDS and goes out as 16-byte stores from byte b0 * 18 / b0 * 17 on (b0 a multiple of 256: 16-byte aligned when `blocks`
// is); the partial 16-byte chunk that may end the last tile goes out as 2-byte stores -- the encoder's output scheme.
constexpr int PK_TILE = 256, PK_MAX_GRID = 4096;

template <bool XS>
__global__ __launch_bounds__(256) void iq4_pack_kernel(const uint8_t* __restrict__ qweight, const uint16_t* __restrict__ d,
                                                       const uint8_t* __restrict__ ls, const int32_t* __restrict__ row_src,
                                                       int64_t nblocks, uint32_t nbr, uint8_t* __restrict__ blocks) {
    constexpr int BB = XS ? 17 : 18;  // output bytes per 32-value block (136 / 8, 18)
    __shared__ __attribute__((aligned(16))) uint8_t img[PK_TILE * BB];
    const int tid = threadIdx.x;
    for (int64_t b0 = (int64_t)blockIdx.x * PK_TILE; b0 < nblocks; b0 += (int64_t)gridDim.x * PK_TILE) {
        const int nb = (int)((nblocks - b0) < PK_TILE ? (nblocks - b0) : PK_TILE);
        const int64_t r0 = b0 / nbr;
        const uint32_t j0 = (uint32_t)(b0 - r0 * nbr);
        if (tid < nb) {
            const uint32_t jl = j0 + (uint32_t)tid, dr = jl / nbr, j = jl - dr * nbr;
            const int64_t r = r0 + dr, sr = row_src ? (int64_t)row_src[r] : r;
            const uint4* qp = reinterpret_cast<const uint4*>(qweight + (sr * nbr + j) * 32);
            const uint4 lo = qp[0], hi = qp[1];  // value k in the low nibble of byte k, value k + 16 in the high one
            const uint32_t qs[4] = {(lo.x & 0x0f0f0f0fu) | (hi.x & 0x0f0f0f0fu) << 4, (lo.y & 0x0f0f0f0fu) | (hi.y & 0x0f0f0f0fu) << 4,
                                    (lo.z & 0x0f0f0f0fu) | (hi.z & 0x0f0f0f0fu) << 4, (lo.w & 0x0f0f0f0fu) | (hi.w & 0x0f0f0f0fu) << 4};
            if constexpr (!XS) {
                uint16_t* ob = reinterpret_cast<uint16_t*>(img + tid * 18);
                ob[0] = d[sr * nbr + j];
#pragma unroll
                for (int k = 0; k < 4; ++k) ob[1 + 2 * k] = (uint16_t)(qs[k] & 0xffffu), ob[2 + 2 * k] = (uint16_t)(qs[k] >> 16);
            } else {
                uint8_t* sb = img + (tid >> 3) * 136;
                if ((tid & 7) == 0) {  // (j is a multiple of 8 here)
                    const uint8_t* lp = ls + sr * nbr + j;
                    uint32_t scales_h = 0, scales_l = 0;
#pragma unroll
                    for (int ib = 0; ib < 8; ++ib) {
                        const uint32_t v = lp[ib];
                        scales_h |= ((v >> 4) & 3u) << (2 * ib);
                        scales_l |= (v & 15u) << (4 * ib);  // byte ib / 2, nibble ib % 2
                    }
                    *reinterpret_cast<uint2*>(sb) = make_uint2((uint32_t)d[sr * (nbr / 8) + j / 8] | (scales_h << 16), scales_l);
                }
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
        __syncthreads();  // the next turn writes `img`
    }
}

}  // namespace

// the lazy scale step of the 256-column group at column a (a % 256 == 0): called by the walk, whose checks have passed
int launch_iq4_scale_step(const float* W, int64_t R, int64_t C, int64_t a, bool xs, const float* importance, uint16_t* d,
                          uint8_t* ls, float* step, float* istep, hipStream_t st) {
    const int64_t nbr = C / 32, b = a / 32;
    const dim3 grid((unsigned)((R + SS_ROWS - 1) / SS_ROWS));
    const float* imp = importance ? importance + a : nullptr;
    ProfScope ps(PT_SCALE_SEARCH, st);
    if (xs)
        hipLaunchKernelGGL(iq4_scale_step_kernel<true>, grid, dim3(256), 0, st, W + a, R, C, imp, d + a / 256, C / 256, ls + b,
                           step + b, istep + b, nbr);
    else
        hipLaunchKernelGGL(iq4_scale_step_kernel<false>, grid, dim3(256), 0, st, W + a, R, C, imp, d + b, nbr, (uint8_t*)nullptr,
                           step + b, istep + b, nbr);
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // namespace gq

using namespace gq;

extern "C" {

int gq_gptq_quantize_iq4(float* W, const float* U, int64_t R, int64_t C, int q_type, int block_size, const float* importance,
                         uint8_t* qweight, uint16_t* d, uint8_t* ls, float* step, float* istep, void* ws, size_t ws_bytes,
                         void* stream) {
    if (int rc = options_ok()) return rc;
    return gptq_quantize_iq4(W, U, R, C, q_type, block_size, importance, qweight, d, ls, step, istep, ws, ws_bytes,
                             (hipStream_t)stream);
}

int gq_pack_iq4(int q_type, int64_t R, int64_t C, const uint8_t* qweight, const uint16_t* d, const uint8_t* ls,
                const int32_t* row_src, uint8_t* blocks, void* stream) {
    if (int rc = options_ok()) return rc;
    if (q_type != GQ_IQ4_NL && q_type != GQ_IQ4_XS)
        GQ_FAIL(GQ_E_BAD_TYPE, "gq_pack_iq4: q_type %d is neither GQ_IQ4_NL (20) nor GQ_IQ4_XS (23)", q_type);
    const bool xs = q_type == GQ_IQ4_XS;
    if (R < 1 || C < 32 || C > 0x7fffffff || C % (xs ? 256 : 32))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_pack_iq4: R=%ld C=%ld (R >= 1, C %% %d == 0, 32 <= C < 2^31)", (long)R, (long)C, xs ? 256 : 32);
    if (!qweight || !d || !blocks || (xs && !ls)) GQ_FAIL(GQ_E_NULL, "gq_pack_iq4: null pointer");
    if (!aligned(qweight, 16) || !aligned(blocks, 16)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_pack_iq4: qweight and blocks must be 16-byte aligned");
    if (!aligned(d, 2) || !aligned(row_src, 4)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_pack_iq4: d not 2-byte or row_src not 4-byte aligned");
    const uint32_t nbr = (uint32_t)(C / 32);
    if (R > INT64_MAX / 64 / nbr) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_pack_iq4: R=%ld C=%ld is too large", (long)R, (long)C);
    const int64_t nblocks = R * nbr, tiles = (nblocks + PK_TILE - 1) / PK_TILE;
    const dim3 grid((unsigned)(tiles < PK_MAX_GRID ? tiles : PK_MAX_GRID));
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PT_PACK, st);
    if (xs) hipLaunchKernelGGL(iq4_pack_kernel<true>, grid, dim3(256), 0, st, qweight, d, ls, row_src, nblocks, nbr, blocks);
    else hipLaunchKernelGGL(iq4_pack_kernel<false>, grid, dim3(256), 0, st, qweight, d, ls, row_src, nblocks, nbr, blocks);
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
