// gq_gemv_a8_core.hpp -- the one text of the dot4 GEMV on int8 activations: what a lane loads of a superblock (piece,
// load_raw, load_item), the integer part of a lane against the quantized image in LDS (lane_dots) and the walk of a wave over
// its rows (row_walk).  gq_gemv_a8.hip (K37: the rows of one weight, token t = row t of x and of y), gq_moe_gemv_a8.hip
// (K38: the rows of one expert's slice of a stacked tensor, token t = the t-th matching pair of a pass) and
// gq_gemv_group_a8.hip (K39: the rows of up to four weights of one input on a partitioned grid) include it, so for one
// weight row and one quantized input row the three kernels run the same instructions in the same order: row p of K38's y is
// bit for bit K37's result at T = 1 on that slice and that input row.  A token's accumulator is touched by no other token, so
// the number of tokens of an instance does not change a token's bits either.  The form is described at the head of
// gq_gemv_a8.hip.  Device code only.
#pragma once

#include "gq_gemv_a8_plan.hpp"
#include "gq_qgemm_a8_core.hpp"

namespace gq {
namespace gemva8 {

using namespace a8core;  // quantize_superblock, signed4, A8<QT>; through it blockdec's loads and layouts

typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));  // four dwords at a 4-byte aligned address

constexpr int NT = 64 * GEMV_A8_NW;
constexpr uint32_t M01 = 0x01010101u, M03 = 0x03030303u, M0F = 0x0f0f0f0fu;

// registers of a lane's share of one superblock, as loaded
template <int QT> constexpr int NRAW = QT == GQ_Q2_K ? 7 : QT == GQ_Q3_K ? 12 : QT == GQ_Q4_K ? 12 : QT == GQ_Q5_K ? 20 : QT == GQ_Q6_K ? 15 : 17;
// bytes of a row's share of one superblock
template <int QT> constexpr int ROWB = QL<QT>::ROWB;

__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int c) { return __builtin_amdgcn_sdot4((int)a, (int)b, c, false); }

// N dwords from a (a - s is 4-byte aligned, s = 0 or 2): see the head of gq_gemv_a8.hip
template <int N>
__device__ __forceinline__ void piece(const uint8_t* a, uint32_t s, uint32_t* w) {
    const uint8_t* q = a - s;
    uint32_t d[N + 1];
    d[0] = s ? (uint32_t)ld2(a) << 16 : ld4(a);
#pragma unroll
    for (int i = 1; i < N; ++i) d[i] = ld4(q + 4 * i);
    d[N] = s ? (uint32_t)ld2(q + 4 * N) : 0u;
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], s);
}

// lane p's share of the superblock at A
template <int QT>
__device__ __forceinline__ void load_raw(const uint8_t* A, int p, uint32_t* w) {
    const int ch = p >> 1, l0 = 16 * (p & 1);
    const uint32_t s = (uint32_t)reinterpret_cast<uintptr_t>(A) & 2u;  // every piece begins at a multiple of 4 from A
    if constexpr (QT == GQ_Q4_K) {  // {d, dmin, scales[12]} | qs[32 p .. + 31]
        ld16(A, w), ld16(A + 16 + 32 * p, w + 4), ld16(A + 32 + 32 * p, w + 8);
    } else if constexpr (QT == GQ_Q5_K) {  // header | qh[32] | qs[32 p .. + 31]
        ld16(A, w), ld16(A + 16, w + 4), ld16(A + 32, w + 8), ld16(A + 48 + 32 * p, w + 12), ld16(A + 64 + 32 * p, w + 16);
    } else if constexpr (QT == GQ_Q2_K) {  // qs[32 ch + l0 .. + 15] | scales[8 ch .. + 7] | {d, dmin}
        const u32x4a4 v = *reinterpret_cast<const u32x4a4*>(A + 16 + 16 * p);
        w[0] = v[0], w[1] = v[1], w[2] = v[2], w[3] = v[3];
        w[4] = ld4(A + 8 * ch), w[5] = ld4(A + 8 * ch + 4), w[6] = ld4(A + 80);
    } else if constexpr (QT == GQ_Q3_K) {  // qs[32 ch + l0 .. + 15] | hmask[l0 .. + 15] | scales[12] | d
        piece<4>(A + 32 + 16 * p, s, w), piece<4>(A + l0, s, w + 4), piece<3>(A + 96, s, w + 8);
        w[11] = ld2(A + 108);
    } else if constexpr (QT == GQ_Q6_K) {  // ql[64 ch + l0 ..] | ql[64 ch + 32 + l0 ..] | qh[32 ch + l0 ..] | scales[8 ch .. + 7] | d
        piece<4>(A + 64 * ch + l0, s, w), piece<4>(A + 64 * ch + 32 + l0, s, w + 4), piece<4>(A + 128 + 16 * p, s, w + 8);
        piece<2>(A + 192 + 8 * ch, s, w + 12);
        w[14] = ld2(A + 208);
    } else {  // Q8_0: blocks 2 p and 2 p + 1 as they lie, {d, qs[32]} {d, qs[32]}
        piece<17>(A + 68 * p, s, w);
    }
}

// lane group g4's superblock of step `st` of row r (r < R) of a weight of nsb superblocks per row, if the row has one;
// row_at(r): the first byte of the packed row that holds row r
template <int QT, class RowAt>
__device__ __forceinline__ void load_item(RowAt row_at, int nsb, int g4, int p, uint32_t* w, int64_t r, int st) {
    const int j = GEMV_A8_STEP * st + g4;
    if (j < nsb) load_raw<QT>(row_at(r) + (int64_t)j * ROWB<QT>, p, w);
}
// row_at of a weight whose row r is packed row row_of(r) of `blocks`
template <int QT, class RowOf>
__device__ __forceinline__ auto rows_of(const uint8_t* __restrict__ blocks, RowOf row_of, int nsb) {
    return [=](int64_t r) { return blocks + (int64_t)row_of(r) * nsb * ROWB<QT>; };
}

__device__ __forceinline__ u32x4 lds16(const int8_t* p) { return *reinterpret_cast<const u32x4*>(p); }
__device__ __forceinline__ int dot16(const uint32_t* c, u32x4 x, int acc) {
    return dot4(c[3], x[3], dot4(c[2], x[2], dot4(c[1], x[1], dot4(c[0], x[0], acc))));
}

// The integer part of a lane for superblock j and TT tokens: w as loaded, X = the image's codes at superblock j of token 0
// (token t at X + t C), BS = the image's group sums at superblock j of token 0 (token t at BS + t C / 16).
// K-quants: isum[t], msum[t] of the lane's groups and (d, dmin); Q8_0: fs[t] = d_b float(isum_b) summed over the lane's two blocks.
template <int QT, int TT>
__device__ __forceinline__ void lane_dots(const uint32_t* w, int p, const int8_t* X, const int16_t* BS, int C, int* isum, int* msum,
                                          float* fs, float& d, float& dmin) {
    const int ch = p >> 1, hb = p & 1, l0 = 16 * hb;
    uint32_t c[16];  // the lane's 64 codes as int8 operands: c[4 k + i] = bytes 4 i .. 4 i + 3 of its k-th run of 16
    int sc[4], mn[4] = {0, 0, 0, 0};
    d = dmin = 0.f;
    if constexpr (QT == GQ_Q4_K || QT == GQ_Q5_K) {  // runs 0, 1: group 2 p; runs 2, 3: group 2 p + 1
        const uint32_t* q = w + (QT == GQ_Q5_K ? 12 : 4);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            c[i] = q[i] & M0F, c[8 + i] = (q[i] >> 4) & M0F;
            if constexpr (QT == GQ_Q5_K) c[i] |= ((w[4 + i] >> (2 * p)) & M01) << 4, c[8 + i] |= ((w[4 + i] >> (2 * p + 1)) & M01) << 4;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {  // get_scale_min_k4 on the 12 scale bytes (group_scale's text, from registers)
            const int g = 2 * p + u, sh = 8 * (g & 3);
            const int s6 = (w[1] >> sh) & 63, m6 = (w[2] >> sh) & 63;
            const int s4 = ((w[3] >> sh) & 0xF) | (((w[1] >> (sh + 6)) & 3) << 4), m4 = ((w[3] >> (sh + 4)) & 0xF) | (((w[2] >> (sh + 6)) & 3) << 4);
            sc[u] = g < 4 ? s6 : s4, mn[u] = g < 4 ? m6 : m4;
        }
        d = h2f((uint16_t)w[0]), dmin = h2f((uint16_t)(w[0] >> 16));
    } else if constexpr (QT == GQ_Q8_0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], 2), c[8 + i] = w[9 + i];
    } else {  // run k = quarter k of the lane's 16 plane bytes = group 8 ch + 2 k + hb
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int bsh = 8 * (2 * (k & 1) + hb);  // the group's byte within its scale word
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (QT == GQ_Q2_K) c[4 * k + i] = (w[i] >> (2 * k)) & M03;
                else if constexpr (QT == GQ_Q3_K) c[4 * k + i] = signed4<QT>(((w[i] >> (2 * k)) & M03) | (((w[4 + i] >> (4 * ch + k)) & M01) << 2));
                else c[4 * k + i] = signed4<QT>(((w[4 * (k & 1) + i] >> (4 * (k >> 1))) & M0F) | (((w[8 + i] >> (2 * k)) & M03) << 4));
            }
            if constexpr (QT == GQ_Q2_K) {
                const uint32_t v = (w[4 + (k >> 1)] >> bsh) & 0xffu;
                sc[k] = v & 0xF, mn[k] = v >> 4;
            } else if constexpr (QT == GQ_Q3_K) {  // six bits: a nibble of scales[0 .. 7], two bits of scales[8 .. 11]
                const uint32_t lo = (w[8 + (k >> 1)] >> (bsh + 4 * ch)) & 0xF, hi = (w[10] >> (bsh + 2 * (2 * ch + (k >> 1)))) & 3;
                sc[k] = (int)(lo | (hi << 4)) - 32;
            } else {
                sc[k] = (int)(int8_t)(w[12 + (k >> 1)] >> bsh);
            }
        }
        if constexpr (QT == GQ_Q2_K) d = h2f((uint16_t)w[6]), dmin = h2f((uint16_t)(w[6] >> 16));
        else d = h2f((uint16_t)w[QT == GQ_Q3_K ? 11 : 14]);
    }
#pragma unroll
    for (int t = 0; t < TT; ++t) {
        const int8_t* Xt = X + t * C;
        if constexpr (A8<QT>::G32) {  // 64 contiguous codes of the token
            const int a = dot16(c + 4, lds16(Xt + 64 * p + 16), dot16(c, lds16(Xt + 64 * p), 0));
            const int b = dot16(c + 12, lds16(Xt + 64 * p + 48), dot16(c + 8, lds16(Xt + 64 * p + 32), 0));
            if constexpr (QT == GQ_Q8_0) {
                fs[t] = h2f((uint16_t)w[0]) * (float)a + h2f((uint16_t)(w[8] >> 16)) * (float)b;
            } else {
                const uint2 bs = *reinterpret_cast<const uint2*>(BS + t * (C / 16) + 4 * p);  // the sums of the lane's four 16s
                isum[t] = sc[0] * a + sc[1] * b;
                msum[t] = mn[0] * ((int)(int16_t)bs.x + (int)(int16_t)(bs.x >> 16)) + mn[1] * ((int)(int16_t)bs.y + (int)(int16_t)(bs.y >> 16));
            }
        } else {
            int is = 0, ms = 0;
            u32x4 bs = {0u, 0u, 0u, 0u};
            if constexpr (QT == GQ_Q2_K) bs = *reinterpret_cast<const u32x4*>(BS + t * (C / 16) + 8 * ch);  // groups 8 ch .. + 7
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                is += sc[k] * dot16(c + 4 * k, lds16(Xt + 128 * ch + 32 * k + l0), 0);
                if constexpr (QT == GQ_Q2_K) ms += mn[k] * (int)(int16_t)(bs[k] >> (16 * hb));
            }
            isum[t] = is, msum[t] = ms;
        }
    }
}

// The prologue of a workgroup of NT threads: the image of T tokens at a8_img, [codes T C | group sums of 16, int16,
// T C / 8 | steps, fp32, T C / 64], its first `tot` superblocks written with a8core::quantize_superblock, 32 per turn.
// src(sbi): where the 256 values of image superblock sbi begin in x, in elements.  x_up != NULL: the value is
// silu_mul_rounded(x, x_up) of the two elements there.  The caller's barrier follows.
template <class Src>
__device__ __forceinline__ void quantize_image(int T, int tot, int C, Src src, const uint16_t* __restrict__ x,
                                               const uint16_t* __restrict__ x_up, int bf16, uint8_t* a8_img) {
    const int tid = threadIdx.x;
    int8_t* sxq = reinterpret_cast<int8_t*>(a8_img);
    int16_t* sbs = reinterpret_cast<int16_t*>(a8_img + gemv_a8_off_bsum(T, C));
    float* sxd = reinterpret_cast<float*>(a8_img + gemv_a8_off_d(T, C));
    for (int s0 = 0; s0 < tot; s0 += NT / 32) {
        const int sbi = s0 + (tid >> 5), piece8 = tid & 31;
        const bool on = sbi < tot;  // (a whole half wave is on or off)
        uint4 raw = make_uint4(0, 0, 0, 0), rup = raw;
        if (on) {
            const int64_t at = src(sbi) + piece8 * 8;
            raw = *reinterpret_cast<const uint4*>(x + at);
            if (x_up) rup = *reinterpret_cast<const uint4*>(x_up + at);
        }
        const uint32_t xw[4] = {raw.x, raw.y, raw.z, raw.w}, uw[4] = {rup.x, rup.y, rup.z, rup.w};
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint16_t b = (uint16_t)(xw[k >> 1] >> (16 * (k & 1)));
            v[k] = bf16 ? bf2f(b) : h2f(b);
            if (x_up) {
                const uint16_t ub = (uint16_t)(uw[k >> 1] >> (16 * (k & 1)));
                v[k] = bf16 ? silu_mul_rounded<true>(v[k], bf2f(ub)) : silu_mul_rounded<false>(v[k], h2f(ub));
            }
        }
        quantize_superblock(v, on, sbi, piece8, sxq, sxd, sbs);
    }
}

// The walk of a wave over its rows r, next(r), next(next(r)), .. (< R) against the image of TT tokens at a8_img, after the
// barrier that follows the prologue.  row_at: load_item's.  cur: the wave's share of step 0 of row r, loaded before the
// prologue (load_item).  done(t, r, v): called by every lane at the end of row r with token t's sum v, the same in all 64
// lanes and not yet rounded; it rounds and stores (K37, K38: lane t, once, to y) or keeps (K39's gate rows).
template <int QT, int TT, class RowAt, class Next, class Done>
__device__ __forceinline__ void row_walk(RowAt row_at, int64_t R, int C, int64_t r, Next next, uint32_t (&cur)[NRAW<QT>],
                                         const uint8_t* a8_img, Done done) {
    constexpr int NW = NRAW<QT>;
    const int lane = threadIdx.x & 63, p = lane & 3, g4 = lane >> 2;
    const int nsb = C / 256, nsteps = (nsb + GEMV_A8_STEP - 1) / GEMV_A8_STEP;
    const int8_t* sxq = reinterpret_cast<const int8_t*>(a8_img);
    const int16_t* sbs = reinterpret_cast<const int16_t*>(a8_img + gemv_a8_off_bsum(TT, C));
    const float* sxd = reinterpret_cast<const float*>(a8_img + gemv_a8_off_d(TT, C));
    int step = 0;
    float facc[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) facc[t] = 0.f;
#pragma unroll 1
    while (r < R) {
        int nstep = step + 1;
        int64_t nr = r;
        if (nstep == nsteps) nstep = 0, nr = next(r);
        uint32_t nxt[NW] = {};
        if (nr < R) load_item<QT>(row_at, nsb, g4, p, nxt, nr, nstep);

        const int j = GEMV_A8_STEP * step + g4;
        const bool active = j < nsb;
        const int jc = active ? j : 0;  // (an idle lane group reads superblock 0 of the image and drops the result)
        int isum[TT], msum[TT];
        float fs[TT], d, dmin;
        lane_dots<QT, TT>(cur, p, sxq + 256 * jc, sbs + 16 * jc, C, isum, msum, fs, d, dmin);
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            float v;
            if constexpr (QT == GQ_Q8_0) {
                v = fs[t];
                v += __shfl_xor(v, 1);
                v += __shfl_xor(v, 2);
            } else {
                int is = isum[t];
                is += __shfl_xor(is, 1);
                is += __shfl_xor(is, 2);
                v = d * (float)is;
                if constexpr (A8<QT>::MINS) {
                    int ms = msum[t];
                    ms += __shfl_xor(ms, 1);
                    ms += __shfl_xor(ms, 2);
                    v = v - dmin * (float)ms;
                }
            }
            const float term = sxd[t * nsb + jc] * v;
            facc[t] += active ? term : 0.f;
        }

        if (step == nsteps - 1) {  // the row is complete: the sixteen lane groups, then one rounding
#pragma unroll
            for (int t = 0; t < TT; ++t) {
                float v = facc[t];
#pragma unroll
                for (int m = GEMV_A8_LANES; m < 64; m <<= 1) v += __shfl_xor(v, m);
                done(t, r, v);
                facc[t] = 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) cur[i] = nxt[i];
        r = nr, step = nstep;
    }
}

// done of a walk that stores: lane t writes token t of row r, rounded once, to row yrow(t) of y [., R] (negative: an idle
// column, not stored)
template <class YRow>
__device__ __forceinline__ auto store_rows(uint16_t* __restrict__ y, int64_t R, int bf16, YRow yrow) {
    const int lane = threadIdx.x & 63;
    return [=](int t, int64_t r, float v) {
        const int64_t yr = yrow(t);
        if (lane == t && yr >= 0) y[yr * R + r] = bf16 ? f2bf(v) : f2h(v);
    };
}
// next of a walk whose rows lie `stride` apart
__device__ __forceinline__ auto rows_apart(int64_t stride) {
    return [=](int64_t r) { return r + stride; };
}

}  // namespace gemva8
}  // namespace gq
