// gq_qgemm_a8_core.hpp -- the one text of the packed tile GEMM on int8 activations and of the activation quantizer's rule.
//   tile_pass_a8        staging, K loop and epilogue of a workgroup of 4 waves that owns [TT = 128 tokens, TR = 128 rows]
//   quantize_superblock 8 values of a lane -> codes, group sums and the step of the superblock its 32 lanes own
//   silu_mul_rounded    SwiGLU's two roundings in front of that rule, for the quantizers that fuse it
// gq_qgemm_a8.hip (K35: tile token i = token t0 + i of the activations and of y) and gq_moe_gemm_a8.hip (K36: tile token i =
// the i-th pair of an expert's run, its activation row gathered and its y row scattered through a list in LDS) include it, so
// for one weight row and one quantized input row the two GEMMs run the same instructions in the same order: per superblock an
// exact integer part, then a fixed fp32 sequence, added in ascending superblock order into an accumulator no other token
// touches -- the same bits, whatever the token's place in the tile and the other tokens are.  The form is described at the
// head of gq_qgemm_a8.hip.
// Device code only: the entry points' type dispatch and operand checks are search/gq_block_host.hpp's.
#pragma once
#include <float.h>
#include <math.h>

#include "gq_qgemm_core.hpp"

namespace gq {
namespace a8core {

using namespace gemmcore;  // TR, u32x4 and, through it, blockdec's layouts and code extraction

typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int TT = 128;  // tokens of a tile

template <int QT> struct A8 {
    static constexpr bool G32 = QT == GQ_Q4_K || QT == GQ_Q5_K || QT == GQ_Q8_0;   // 32 values per MFMA (else 16)
    static constexpr bool MINS = QT == GQ_Q2_K || QT == GQ_Q4_K || QT == GQ_Q5_K;
    static constexpr bool FOLD = QT == GQ_Q2_K;                                    // the scale is folded into the operand
    static constexpr int NG = G32 ? 8 : 16;                                        // MFMA groups of a superblock
    static constexpr int PT = 4;  // token tiles (of 32) that go through a superblock's groups together: all of the wave's
    static constexpr int PITCH = G32 ? 272 : 264;                                  // bytes of a token in the xq image
    static constexpr uint32_t OFF4 = QT == GQ_Q3_K ? 0x04040404u : QT == GQ_Q6_K ? 0x20202020u : 0u;  // stored code - OFF = w
};

constexpr bool a8_type(int q) { return q == GQ_Q8_0 || (q >= GQ_Q2_K && q <= GQ_Q6_K); }

// four stored codes (each below 128) minus their offset, as four int8: no borrow crosses a byte
template <int QT>
__device__ __forceinline__ uint32_t signed4(uint32_t c) {
    if constexpr (A8<QT>::OFF4 != 0) return ((c | 0x80808080u) - A8<QT>::OFF4) ^ 0x80808080u;
    else return c;
}

__device__ __forceinline__ i32x16 mfma16(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, i32x16 c) {
    const long a = (long)(((uint64_t)a1 << 32) | a0), b = (long)(((uint64_t)b1 << 32) | b0);
    return __builtin_amdgcn_mfma_i32_32x32x16_i8(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ i32x16 mfma32(u32x4 a, u32x4 b, i32x16 c) {
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b), c, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------ the quantizer's rule
// The 8 values v of lane `piece` of superblock sbi (32 consecutive lanes own it; `on` is the same in all of them, so the
// exchanges stay inside the half wave): the maximum through five cross-lane exchanges, 8 codes as one 8-byte store, a group
// sum from two lanes, the step from lane 0.
__device__ __forceinline__ void quantize_superblock(const float v[8], bool on, int64_t sbi, int piece, int8_t* __restrict__ xq,
                                                    float* __restrict__ xd, int16_t* __restrict__ xbsum) {
    float amax = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) amax = fmaxf(amax, fabsf(v[k]));  // (fmaxf skips a NaN)
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) amax = fmaxf(amax, __shfl_xor(amax, m));
    float inv = 127.f / amax, d = amax / 127.f;
    if (amax == 0.f || !(inv <= FLT_MAX)) inv = 0.f, d = 0.f;
    int s = 0;
    uint32_t o[2] = {0u, 0u};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float q = rintf(v[k] * inv);
        q = q != q ? 0.f : fminf(fmaxf(q, -127.f), 127.f);
        const int qi = (int)q;
        s += qi;
        o[k >> 2] |= (uint32_t)(qi & 0xff) << (8 * (k & 3));
    }
    s += __shfl_xor(s, 1);
    if (on) {
        *reinterpret_cast<uint2*>(xq + sbi * 256 + piece * 8) = make_uint2(o[0], o[1]);
        if (!(piece & 1)) xbsum[sbi * 16 + (piece >> 1)] = (int16_t)s;
        if (piece == 0) xd[sbi] = d;
    }
}

// gq_fwd_silu_mul's operations on one element (fwd_silu_mul_kernel's): ATen's silu g / (1 + exp(-g)) in fp32, rounded to the
// 16-bit type, times up, rounded again -> the value the quantizer sees.  gq_silu_mul_quantize_act_q8 (K36) and the prologue of
// gq_gemv_packed_experts_a8 (K38) run this text.
template <bool BF16>
__device__ __forceinline__ float silu_mul_rounded(float g, float u) {
    const float sf = g / (1.0f + expf(-g));
    const float s = BF16 ? bf2f(f2bf(sf)) : h2f(f2h(sf));
    const float hf = s * u;
    return BF16 ? bf2f(f2bf(hf)) : h2f(f2h(hf));
}

// ------------------------------------------------------------------------------------------------ the GEMM
// what a thread holds of the next superblock's activations while the current one is multiplied
struct Prefetch {
    u32x4 xr[8];  // piece p = tid + 256 i of the xq tile: token p >> 4, 16-byte piece p & 15
    u32x4 bs;     // 8 group sums of token tid >> 1, half tid & 1
    float d;      // xd of token tid (tid < TT)
};

// xrow(i): the activation row of tile token i, negative when the tile has no such token (staged as zeros).  The three loads
// of a token address through the same row.
template <bool MINS, class XRow>
__device__ __forceinline__ void prefetch(Prefetch& f, const int8_t* __restrict__ xq, const float* __restrict__ xd,
                                         const int16_t* __restrict__ xbsum, int64_t C, XRow xrow, int64_t j) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int p = tid + 256 * i;
        const int64_t t = xrow(p >> 4);
        f.xr[i] = t >= 0 ? *reinterpret_cast<const u32x4*>(xq + t * C + 256 * j + 16 * (p & 15)) : u32x4{0, 0, 0, 0};
    }
    if constexpr (MINS) {
        const int64_t t = xrow(tid >> 1);
        f.bs = t >= 0 ? *reinterpret_cast<const u32x4*>(xbsum + t * (C / 16) + 16 * j + 8 * (tid & 1)) : u32x4{0, 0, 0, 0};
    }
    f.d = 0.f;
    if (tid < TT) {
        const int64_t t = xrow(tid);
        if (t >= 0) f.d = xd[t * (C / 256) + j];
    }
}

template <int QT>
__device__ __forceinline__ void commit(const Prefetch& f, uint8_t* sx, uint8_t* sbl, uint8_t* sbh, float* sxd) {
    using P = A8<QT>;
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int p = tid + 256 * i;
        uint8_t* dst = sx + (p >> 4) * P::PITCH + 16 * (p & 15);
        if constexpr (P::PITCH % 16 == 0) {
            *reinterpret_cast<u32x4*>(dst) = f.xr[i];
        } else {  // the 264-byte pitch keeps 8-byte alignment only
            *reinterpret_cast<uint2*>(dst) = make_uint2(f.xr[i][0], f.xr[i][1]);
            *reinterpret_cast<uint2*>(dst + 8) = make_uint2(f.xr[i][2], f.xr[i][3]);
        }
    }
    if constexpr (P::MINS) {  // xbsum = 64 hi + lo, lo in [0, 63], hi in [-32, 31]: one byte plane each
        uint32_t lo[2] = {0u, 0u}, hi[2] = {0u, 0u};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int v = (int)(int16_t)(f.bs[k >> 1] >> (16 * (k & 1)));
            lo[k >> 2] |= (uint32_t)(v & 63) << (8 * (k & 3));
            hi[k >> 2] |= (uint32_t)((v >> 6) & 0xff) << (8 * (k & 3));
        }
        *reinterpret_cast<uint2*>(sbl + (tid >> 1) * 16 + 8 * (tid & 1)) = make_uint2(lo[0], lo[1]);
        *reinterpret_cast<uint2*>(sbh + (tid >> 1) * 16 + 8 * (tid & 1)) = make_uint2(hi[0], hi[1]);
    }
    if (tid < TT) sxd[tid] = f.d;
}

// Superblock j of the tile's nr packed rows into their slots (K21's layout: QL<QT>), with loads of the type's natural width that
// cover exactly the blocks' bytes.  (K21's stage_rows keeps eight loads in an array, which this kernel's register budget sends to
// scratch for the 16-byte types; four loads in flight per turn stay in registers.)
template <int QT>
__device__ __forceinline__ void stage_packed(const uint8_t* __restrict__ blocks, const int64_t* sbase, int64_t j, int nr, uint8_t* sb) {
    using Q = QL<QT>;
    using U = typename Unit<Q::AL>::T;
    const int n = nr * Q::UPR;
#pragma unroll 4
    for (int u = threadIdx.x; u < n; u += 256) {
        const int r = u / Q::UPR, o = u - r * Q::UPR;
        *reinterpret_cast<U*>(sb + r * Q::SLOT + Q::lds_off(o)) = *reinterpret_cast<const U*>(blocks + sbase[r] + j * Q::ROWB + o * Q::AL);
    }
}

// a lane's weight operand of MFMA group g: its row's slot B, lane half h
template <int QT>
__device__ __forceinline__ u32x4 weight_operand(const uint8_t* B, int g, int h, int sc) {
    using P = A8<QT>;
    uint32_t c[4];
    if constexpr (QT == GQ_Q8_0) {
        ld16(B + 16 + 32 * g + 16 * h, c);
        return u32x4{c[0], c[1], c[2], c[3]};
    } else if constexpr (P::G32) {
        codes16<QT>(B, 2 * g + h, c);
        return u32x4{c[0], c[1], c[2], c[3]};
    } else {  // the 8 values of this lane half
        codes16<QT>(B, g, c);
        uint32_t a = signed4<QT>(h ? c[2] : c[0]), b = signed4<QT>(h ? c[3] : c[1]);
        if constexpr (P::FOLD) a *= (uint32_t)sc, b *= (uint32_t)sc;  // every byte stays below 46
        return u32x4{a, b, 0u, 0u};
    }
}

// LDS of a workgroup: the packed slots, the xq image, the two xbsum planes and xd (the caller declares them, with sbase)
template <int QT> struct TileLds {
    static constexpr int SB = TR * QL<QT>::SLOT, SX = TT * A8<QT>::PITCH, PLANE = A8<QT>::MINS ? TT * 16 : 16;
};

// The tile of rows r0 .. r0 + nr - 1 (sbase[r] = byte offset of the row's first block; the caller has written it, no barrier
// needed yet) and of ntt token tiles of 32.  xrow(i) / yrow(i): the activation row and the row of y of tile token i, negative:
// none (staged as zeros / not stored); both must be readable before the call.
template <int QT, class XRow, class YRow>
__device__ __forceinline__ void tile_pass_a8(const uint8_t* __restrict__ blocks, const int64_t* sbase, int nr, int ntt, int64_t r0,
                                             int64_t R, int64_t C, const int8_t* __restrict__ xq, const float* __restrict__ xd,
                                             const int16_t* __restrict__ xbsum, XRow xrow, uint16_t* __restrict__ y, int bf16,
                                             YRow yrow, uint8_t* sb, uint8_t* sx, uint8_t* sbl, uint8_t* sbh, float* sxd) {
    using Q = QL<QT>;
    using P = A8<QT>;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int64_t nsb = C / 256;

    float facc[4][16];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int i = 0; i < 16; ++i) facc[tt][i] = 0.f;
    const i32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

    Prefetch pf;
    prefetch<P::MINS>(pf, xq, xd, xbsum, C, xrow, 0);
    __syncthreads();  // sbase
    const uint8_t* B0 = sb + (32 * wave + l31) * Q::SLOT;
    const uint8_t* X0 = sx + l31 * P::PITCH + (P::G32 ? 16 : 8) * h;
#pragma unroll 1
    for (int64_t j = 0; j < nsb; ++j) {
        commit<QT>(pf, sx, sbl, sbh, sxd);
        stage_packed<QT>(blocks, sbase, j, nr, sb);
        __syncthreads();
        if (j + 1 < nsb) prefetch<P::MINS>(pf, xq, xd, xbsum, C, xrow, j + 1);

#pragma unroll
        for (int tb = 0; tb < 4; tb += P::PT) {  // a pass: PT token tiles through all groups, the mins and the float side
            i32x16 isum[P::PT];   // K-quants: sum_g sc_g (w . xq)
            float fs[P::PT][16];  // Q8_0: sum_b d_b float(w . xq)
#pragma unroll
            for (int u = 0; u < P::PT; ++u) {
                isum[u] = zero;
#pragma unroll
                for (int i = 0; i < 16; ++i) fs[u][i] = 0.f;
            }
#pragma unroll
            for (int g = 0; g < P::NG; ++g) {
                int sc = 0, mn = 0;
                if constexpr (QT != GQ_Q8_0) group_scale<QT>(B0, g, sc, mn);
                const u32x4 wb = weight_operand<QT>(B0, g, h, sc);
                const float db = QT == GQ_Q8_0 ? h2f(ld2(B0 + 2 * g)) : 0.f;
#pragma unroll
                for (int u = 0; u < P::PT; ++u)
                    if (tb + u < ntt) {
                        const int tt = tb + u;
                        const uint8_t* px = X0 + 32 * tt * P::PITCH + (P::G32 ? 32 : 16) * g;
                        i32x16 D;
                        if constexpr (P::G32) {
                            D = mfma32(*reinterpret_cast<const u32x4*>(px), wb, zero);
                        } else {
                            const uint2 xa = *reinterpret_cast<const uint2*>(px);
                            D = mfma16(xa.x, xa.y, wb[0], wb[1], P::FOLD ? isum[u] : zero);
                        }
                        if constexpr (QT == GQ_Q8_0) {
#pragma unroll
                            for (int i = 0; i < 16; ++i) fs[u][i] += db * (float)D[i];
                        } else if constexpr (P::FOLD) {
                            isum[u] = D;
                        } else {  // |D| <= 32 * 31 * 127 and |sc| <= 128: both inside 24 bits, the sum inside 32
#pragma unroll
                            for (int i = 0; i < 16; ++i) isum[u][i] += __mul24(sc, D[i]);
                        }
                    }
            }

            uint32_t wm0 = 0u, wm1 = 0u;  // the min of the group that 16-value group 8 h + e lies in, e = 0 .. 7
            if constexpr (P::MINS) {
                constexpr int NGT = Lay<QT>::NG;  // the type's scale groups: 16 (Q2_K) or 8
                uint32_t m[2][2] = {{0u, 0u}, {0u, 0u}};
#pragma unroll
                for (int g16 = 0; g16 < 16; ++g16) {
                    int sc, mn;
                    group_scale<QT>(B0, g16 * NGT / 16, sc, mn);
                    m[g16 >> 3][(g16 >> 2) & 1] |= (uint32_t)mn << (8 * (g16 & 3));
                }
                wm0 = h ? m[1][0] : m[0][0], wm1 = h ? m[1][1] : m[0][1];
            }
            uint16_t dbits = 0, dminbits = 0;
            if constexpr (QT != GQ_Q8_0) block_d<QT>(B0, dbits, dminbits);
            const float d = h2f(dbits), dmin = h2f(dminbits);
#pragma unroll
            for (int u = 0; u < P::PT; ++u)
                if (tb + u < ntt) {
                    const int tt = tb + u;
                    i32x16 msum = zero;
                    if constexpr (P::MINS) {
                        const uint2 xl = *reinterpret_cast<const uint2*>(sbl + (32 * tt + l31) * 16 + 8 * h);
                        const uint2 xh = *reinterpret_cast<const uint2*>(sbh + (32 * tt + l31) * 16 + 8 * h);
                        const i32x16 Dh = mfma16(xh.x, xh.y, wm0, wm1, zero);
                        msum = mfma16(xl.x, xl.y, wm0, wm1, Dh * 64);
                    }
#pragma unroll
                    for (int i4 = 0; i4 < 4; ++i4) {
                        const float4 xdv = *reinterpret_cast<const float4*>(sxd + 32 * tt + 8 * i4 + 4 * h);
                        const float xv[4] = {xdv.x, xdv.y, xdv.z, xdv.w};
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int i = 4 * i4 + k;
                            float v;
                            if constexpr (QT == GQ_Q8_0) v = fs[u][i];
                            else if constexpr (P::MINS) v = d * (float)isum[u][i] - dmin * (float)msum[i];
                            else v = d * (float)isum[u][i];
                            facc[tt][i] += xv[k] * v;
                        }
                    }
                }
        }
        __syncthreads();  // sb, sx and the planes may be overwritten
    }

    const int64_t r = r0 + 32 * wave + l31;
    if (r >= R) return;
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
        if (tt < ntt) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t t = yrow(32 * tt + 8 * (i >> 2) + 4 * h + (i & 3));
                if (t >= 0) y[t * R + r] = bf16 ? f2bf(facc[tt][i]) : f2h(facc[tt][i]);
            }
        }
}

}  // namespace a8core
}  // namespace gq
