// gq_qk_norm_rope.hip -- K32: what a Qwen3 attention layer adds to Llama's between the projections and the attention.
// transformers' Qwen3Attention.forward runs
//     q = q_norm(q_proj(x).view(B, L, Hq, D));  k = k_norm(k_proj(x).view(B, L, Hk, D));  q, k = apply_rotary_pos_emb(q, k, cos, sin)
// -- two Qwen3RMSNorm over head_dim (about six torch elementwise / reduce kernels each, with fp32 round trips of [B, L, H, D])
// and the rotary embedding.  gq_fwd_qk_norm_rope does all of it for both tensors in ONE launch with the same roundings and
// the summation order of ATen's mean (include/gptq_gguf_qknorm.h states the contract).
//
// Lanes: PER = D / 16 lanes own a row; lane l holds x[8 l .. 8 l + 8) and x[D/2 + 8 l .. D/2 + 8 l + 8) -- the two halves the
// rotary embedding pairs, so nothing but the sum of squares crosses lanes.  ATen's order in that layout: the leaves of its
// shuffle-down tree (elements at D = 64, 4-element folds at D = 128 / 256) that a lane holds are consecutive and aligned,
// so the lane sums the lower levels of the tree itself, log2(PER) xor-shuffles finish the tree over each half of the row
// (a + b == b + a bit for bit: both partners of an exchange hold the node), and the two halves are added last.
// A group of PER lanes takes up to HEADS consecutive heads of one token out of its Hq + Hk (q first): the token's cos / sin
// are loaded once for them, and all loads of the group are in flight before the first use.
#include "../../../include/gptq_gguf_qknorm.h"

#include "../gq_common.hpp"
#include "gq_rsqrt_rn.hpp"

namespace gq {
namespace {

constexpr int HEADS = 4;  // heads of one token per lane group

template <bool BF16> __device__ __forceinline__ float ld16(uint16_t v) { return BF16 ? bf2f(v) : h2f(v); }
template <bool BF16> __device__ __forceinline__ uint16_t st16(float f) { return BF16 ? f2bf(f) : f2h(f); }

template <bool BF16> __device__ __forceinline__ void unpack8(const uint4& v, float* f) {
    const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f[2 * e] = ld16<BF16>((uint16_t)(u[e] & 0xffff));
        f[2 * e + 1] = ld16<BF16>((uint16_t)(u[e] >> 16));
    }
}

// the node of ATen's tree over the 8 consecutive elements f[0 .. 8) of a row (pow(2) rounds each square to fp32 first)
template <bool VEC> __device__ __forceinline__ float node8(const float* f) {
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = f[e] * f[e];
    if constexpr (VEC) {  // two leaves, each a vector's four accumulators folded in index order
        return (((s[0] + s[1]) + s[2]) + s[3]) + (((s[4] + s[5]) + s[6]) + s[7]);
    } else {  // eight leaves: three levels of the shuffle-down tree
        return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    }
}

template <bool BF16, int D>
__global__ __launch_bounds__(256) void fwd_qk_norm_rope_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                               const uint16_t* __restrict__ wq, const uint16_t* __restrict__ wk,
                                                               const uint16_t* __restrict__ cs, const uint16_t* __restrict__ sn,
                                                               uint16_t* __restrict__ qo, uint16_t* __restrict__ ko,
                                                               int64_t tokens, int Hq, int Hk, int chunks, float eps, float factor,
                                                               float* __restrict__ stats) {
    constexpr int PER = D / 16, HALF = D / 2;
    constexpr bool VEC = D >= 128;  // Reduce.cuh vectorises the input from 128 values per output on
    const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) / PER;  // (token, chunk of heads)
    if (g >= tokens * chunks) return;  // whole groups leave: the shuffles below stay inside a group
    const int64_t tok = g / chunks;
    const int h0 = (int)(g % chunks) * HEADS, H = Hq + Hk;
    const int d0 = 8 * (int)(threadIdx.x % PER);

    const uint16_t* xin[HEADS];
    uint16_t* xout[HEADS];
    int64_t srow[HEADS];
    uint4 xa[HEADS], xb[HEADS];
#pragma unroll
    for (int i = 0; i < HEADS; ++i) {
        const int h = h0 + i;
        if (h < H) {
            const bool isq = h < Hq;
            const int64_t row = isq ? tok * Hq + h : tok * Hk + (h - Hq);
            xin[i] = (isq ? q : k) + row * D;
            xout[i] = (isq ? qo : ko) + row * D;
            srow[i] = isq ? row : tokens * Hq + row;
            xa[i] = *reinterpret_cast<const uint4*>(xin[i] + d0);
            xb[i] = *reinterpret_cast<const uint4*>(xin[i] + HALF + d0);
        }
    }
    float ca[8], cb[8], sa[8], sb[8], wqa[8], wqb[8], wka[8], wkb[8];
    unpack8<BF16>(*reinterpret_cast<const uint4*>(cs + tok * D + d0), ca);
    unpack8<BF16>(*reinterpret_cast<const uint4*>(cs + tok * D + HALF + d0), cb);
    unpack8<BF16>(*reinterpret_cast<const uint4*>(sn + tok * D + d0), sa);
    unpack8<BF16>(*reinterpret_cast<const uint4*>(sn + tok * D + HALF + d0), sb);
    unpack8<BF16>(*reinterpret_cast<const uint4*>(wq + d0), wqa);
    unpack8<BF16>(*reinterpret_cast<const uint4*>(wq + HALF + d0), wqb);
    unpack8<BF16>(*reinterpret_cast<const uint4*>(wk + d0), wka);
    unpack8<BF16>(*reinterpret_cast<const uint4*>(wk + HALF + d0), wkb);

#pragma unroll
    for (int i = 0; i < HEADS; ++i) {
        const int h = h0 + i;
        if (h >= H) break;  // the same for every lane of the group
        const bool isq = h < Hq;
        float a[8], b[8];
        unpack8<BF16>(xa[i], a);
        unpack8<BF16>(xb[i], b);
        float ta = node8<VEC>(a), tb = node8<VEC>(b);
#pragma unroll
        for (int o = 1; o < PER; o <<= 1) {
            ta = ta + __shfl_xor(ta, o);
            tb = tb + __shfl_xor(tb, o);
        }
        const float var = (ta + tb) * factor;
        const float r = rsqrt_rn(var + eps);
        if (stats && d0 == 0) {
            stats[2 * srow[i]] = var;
            stats[2 * srow[i] + 1] = r;
        }
        uint32_t oa[4], ob[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            uint16_t ra[2], rb[2];
#pragma unroll
            for (int hlf = 0; hlf < 2; ++hlf) {
                const int j = 2 * e + hlf;
                // Qwen3RMSNorm: (x32 * r).to(dtype), then weight * that
                const float ya = ld16<BF16>(st16<BF16>(a[j] * r)), yb = ld16<BF16>(st16<BF16>(b[j] * r));
                const float za = ld16<BF16>(st16<BF16>((isq ? wqa[j] : wka[j]) * ya));
                const float zb = ld16<BF16>(st16<BF16>((isq ? wqb[j] : wkb[j]) * yb));
                // apply_rotary_pos_emb, fwd_rope_kernel's roundings
                const float p0 = ld16<BF16>(st16<BF16>(za * ca[j]));
                const float p1 = ld16<BF16>(st16<BF16>(-zb * sa[j]));
                const float p2 = ld16<BF16>(st16<BF16>(zb * cb[j]));
                const float p3 = ld16<BF16>(st16<BF16>(za * sb[j]));
                ra[hlf] = st16<BF16>(p0 + p1);
                rb[hlf] = st16<BF16>(p2 + p3);
            }
            oa[e] = (uint32_t)ra[0] | ((uint32_t)ra[1] << 16);
            ob[e] = (uint32_t)rb[0] | ((uint32_t)rb[1] << 16);
        }
        *reinterpret_cast<uint4*>(xout[i] + d0) = make_uint4(oa[0], oa[1], oa[2], oa[3]);
        *reinterpret_cast<uint4*>(xout[i] + HALF + d0) = make_uint4(ob[0], ob[1], ob[2], ob[3]);
    }
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_fwd_qk_norm_rope(const void* q, const void* k, const void* wq, const void* wk, const void* cos_, const void* sin_,
                        void* q_out, void* k_out, int64_t tokens, int heads_q, int heads_k, int head_dim, float eps, int dtype,
                        float* stats, void* stream) {
    if (int rc = options_ok()) return rc;
    if (dtype != GQ_F16 && dtype != GQ_BF16) GQ_FAIL(GQ_E_BAD_TYPE, "gq_fwd_qk_norm_rope: dtype %d (fp16 / bf16)", dtype);
    if (!q || !k || !wq || !wk || !cos_ || !sin_ || !q_out || !k_out) GQ_FAIL(GQ_E_NULL, "gq_fwd_qk_norm_rope: null pointer");
    if (head_dim != 64 && head_dim != 128 && head_dim != 256)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_fwd_qk_norm_rope: head_dim=%d (64, 128 or 256)", head_dim);
    if (tokens < 1 || heads_q < 1 || heads_k < 1)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_fwd_qk_norm_rope: tokens=%ld heads_q=%d heads_k=%d (all >= 1)", (long)tokens, heads_q, heads_k);
    if (!aligned(q, 16) || !aligned(k, 16) || !aligned(wq, 16) || !aligned(wk, 16) || !aligned(cos_, 16) || !aligned(sin_, 16) ||
        !aligned(q_out, 16) || !aligned(k_out, 16) || !aligned(stats, 4))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_fwd_qk_norm_rope: a pointer is not 16-byte aligned (stats: 4-byte)");
    const int64_t chunks = ((int64_t)heads_q + heads_k + HEADS - 1) / HEADS;
    const int64_t lanes_per_token = chunks * (head_dim / 16);
    if (tokens > (((int64_t)0x7fffffff * 256) / lanes_per_token))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_fwd_qk_norm_rope: tokens=%ld heads_q=%d heads_k=%d (more rows than one grid takes)", (long)tokens, heads_q, heads_k);
    const dim3 grid((unsigned)((tokens * lanes_per_token + 255) / 256)), block(256);
    const float factor = 1.0f / (float)head_dim;  // ATen's float(rows) / (rows * D): the same value for these D, whatever rows
    hipStream_t st = (hipStream_t)stream;
#define GQ_QKNR(B16, D_)                                                                                                          \
    hipLaunchKernelGGL((fwd_qk_norm_rope_kernel<B16, D_>), grid, block, 0, st, static_cast<const uint16_t*>(q),                   \
                       static_cast<const uint16_t*>(k), static_cast<const uint16_t*>(wq), static_cast<const uint16_t*>(wk),       \
                       static_cast<const uint16_t*>(cos_), static_cast<const uint16_t*>(sin_), static_cast<uint16_t*>(q_out),     \
                       static_cast<uint16_t*>(k_out), tokens, heads_q, heads_k, (int)chunks, eps, factor, stats)
    const bool b16 = dtype == GQ_BF16;
    if (head_dim == 64) { if (b16) GQ_QKNR(true, 64); else GQ_QKNR(false, 64); }
    else if (head_dim == 128) { if (b16) GQ_QKNR(true, 128); else GQ_QKNR(false, 128); }
    else { if (b16) GQ_QKNR(true, 256); else GQ_QKNR(false, 256); }
#undef GQ_QKNR
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
