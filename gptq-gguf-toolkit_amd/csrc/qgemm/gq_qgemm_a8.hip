// gq_qgemm_a8.hip -- K35: the packed-weight forward on int8 activations.
//   gq_quantize_act_q8   x [T, C] fp16 / bf16 -> codes int8 [T, C], a step fp32 per 256 values, group sums int16 per 16 values
//   gq_linear_packed_a8  y = x W^T from those and the packed blocks of W, on the int8 matrix pipe
// The contract of both is include/gptq_gguf_qgemm_a8.h's.  No weight is turned into a float here: a code becomes an int8
// operand with shifts and masks, the products of a scale group are summed exactly by one MFMA, the group's integer scale is
// applied to that int32 tile with one 24-bit multiply-add per element, and the float side (d, dmin, the activation step)
// happens once per superblock of 256 values.
//
// The quantizer.  32 lanes own a superblock: a lane loads 16 bytes (8 values), the maximum goes through five cross-lane
// exchanges, a lane stores its 8 codes as 8 bytes, two lanes make a group sum.  The [T, C] tensor is one run of T * C / 256
// superblocks, 8 to a workgroup; no loop, no workspace.
//
// The GEMM.  A workgroup of 4 waves owns [TT = 128 tokens, TR = 128 rows] and walks C in superblocks (K21's tiling and its
// LDS slots of the packed rows, QL<QT>; staged by stage_packed below).  Wave w owns rows 32 w .. 32 w + 31 and all 128 tokens as four
// 32 x 32 tiles.  The matrix instruction is v_mfma_i32_32x32x{16,32}_i8 with A = x and B = W, so that a lane's 16 results are
// D[token 8 (i >> 2) + 4 (l >> 5) + (i & 3)][row l & 31]: ONE weight row per lane.  Everything that belongs to a row -- its
// LDS slot, d, dmin, the group's scale -- is therefore one value per lane, read once, and the sub-scale step is
// v_mad_i32_i24(sc, D[i], isum[i]) with the same sc for all 16 registers.
//   * Q4_K, Q5_K, Q8_0 (groups of 32): 32x32x32, a lane's operand is 16 bytes = values 32 g + 16 (l >> 5) .. + 15 of its
//     row (codes16 as it stands) and of its token.  One MFMA per group.
//   * Q3_K, Q6_K (groups of 16): 32x32x16, 8 bytes = values 16 g + 8 (l >> 5) .. + 7.  One MFMA per group.
//   * Q2_K (groups of 16): 32x32x16 as well, but the scale is folded into the operand (sc w <= 15 * 3 = 45 fits a byte, one
//     32-bit multiply per word), so the sixteen MFMAs of a superblock chain through the accumulator and no VALU work follows
//     them.  Q3_K is not folded (a per-byte signed product is not one instruction) and Q6_K cannot be (|sc w| up to 4096).
//   * mins (Q2_K, Q4_K, Q5_K): msum = sum_g mn_g xbsum_g is itself a [rows, 16] x [16, tokens] integer product.  xbsum does not
//     fit a byte, so it is staged as two byte planes, xbsum = 64 hi + lo with lo in [0, 63] and hi in [-32, 31], and two
//     32x32x16 MFMAs per token tile and superblock give msum = 64 Dhi + Dlo.  The weight operand holds mn of the group that the
//     16-value group g16 lies in (Q4_K / Q5_K: each min twice).
//   * float side, per superblock and element: xd * (d * float(isum) - dmin * float(msum)); Q8_0 per block: fs += d_b * float(D).
// LDS: the packed slots (K21's), the superblock's xq tile [128 tokens, 256 bytes] at a pitch of 272 (16-byte reads) or 264
// bytes (8-byte reads) so that the 16 (32) tokens of a read fall on different banks, the two xbsum planes [128, 16] and xd:
// 51 KB (Q2_K) .. 78 KB (Q8_0), two workgroups per CU.  The next superblock's xq, xbsum and xd are loaded into registers
// while the MFMAs run.
// Edges: rows >= R are not staged (their slots hold stale bytes that only reach results which are never stored, a lane holds
// one row only), tokens >= T are staged as zeros and not stored.  y is written with 2-byte stores, 32 lanes = 64 contiguous
// bytes of one token's row of y: with one row per lane there are no four consecutive rows in a lane to store 8 bytes wide.
#include "../../../include/gptq_gguf_qgemm_a8.h"

#include <float.h>

#include "../search/gq_block_host.hpp"
#include "gq_qgemm_core.hpp"

namespace gq {
namespace {

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

// ------------------------------------------------------------------------------------------------ the quantizer
template <bool BF16>
__global__ __launch_bounds__(256) void quantize_act_q8_kernel(const uint16_t* __restrict__ x, int64_t nsb, int8_t* __restrict__ xq,
                                                              float* __restrict__ xd, int16_t* __restrict__ xbsum) {
    const int64_t sbi = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 5;
    const int piece = threadIdx.x & 31;
    const bool on = sbi < nsb;  // (a whole half wave is on or off: the exchanges below stay inside it)
    uint4 raw = make_uint4(0, 0, 0, 0);
    if (on) raw = *reinterpret_cast<const uint4*>(x + sbi * 256 + piece * 8);
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
    float v[8], amax = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint16_t b = (uint16_t)(w[k >> 1] >> (16 * (k & 1)));
        v[k] = BF16 ? bf2f(b) : h2f(b);
        amax = fmaxf(amax, fabsf(v[k]));  // (fmaxf skips a NaN)
    }
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

// ------------------------------------------------------------------------------------------------ the GEMM
// what a thread holds of the next superblock's activations while the current one is multiplied
struct Prefetch {
    u32x4 xr[8];  // piece p = tid + 256 i of the xq tile: token p >> 4, 16-byte piece p & 15
    u32x4 bs;     // 8 group sums of token tid >> 1, half tid & 1
    float d;      // xd of token tid (tid < TT)
};

template <bool MINS>
__device__ __forceinline__ void prefetch(Prefetch& f, const int8_t* __restrict__ xq, const float* __restrict__ xd,
                                         const int16_t* __restrict__ xbsum, int64_t C, int64_t T, int64_t t0, int64_t j) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int p = tid + 256 * i;
        const int64_t t = t0 + (p >> 4);
        f.xr[i] = t < T ? *reinterpret_cast<const u32x4*>(xq + t * C + 256 * j + 16 * (p & 15)) : u32x4{0, 0, 0, 0};
    }
    if constexpr (MINS) {
        const int64_t t = t0 + (tid >> 1);
        f.bs = t < T ? *reinterpret_cast<const u32x4*>(xbsum + t * (C / 16) + 16 * j + 8 * (tid & 1)) : u32x4{0, 0, 0, 0};
    }
    f.d = (tid < TT && t0 + tid < T) ? xd[(t0 + tid) * (C / 256) + j] : 0.f;
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

template <int QT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void linear_packed_a8_kernel(
    const uint8_t* __restrict__ blocks, const int32_t* __restrict__ row_src, int64_t R, int64_t C, const int8_t* __restrict__ xq,
    const float* __restrict__ xd, const int16_t* __restrict__ xbsum, int64_t T, uint16_t* __restrict__ y, int bf16, uint32_t n_rt) {
    using Q = QL<QT>;
    using P = A8<QT>;
    __shared__ __attribute__((aligned(16))) uint8_t sb[TR * Q::SLOT];
    __shared__ __attribute__((aligned(16))) uint8_t sx[TT * P::PITCH];
    __shared__ __attribute__((aligned(16))) uint8_t sbl[P::MINS ? TT * 16 : 16], sbh[P::MINS ? TT * 16 : 16];
    __shared__ __attribute__((aligned(16))) float sxd[TT];
    __shared__ int64_t sbase[TR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int64_t r0 = (int64_t)(blockIdx.x % n_rt) * TR, t0 = (int64_t)(blockIdx.x / n_rt) * TT;  // row tiles fastest: they share x
    const int nr = (int)((R - r0) < TR ? (R - r0) : TR), nt = (int)((T - t0) < TT ? (T - t0) : TT), ntt = (nt + 31) >> 5;
    const int64_t nsb = C / 256;
    if (tid < nr) sbase[tid] = (row_src ? (int64_t)row_src[r0 + tid] : r0 + tid) * nsb * Q::ROWB;

    float facc[4][16];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int i = 0; i < 16; ++i) facc[tt][i] = 0.f;
    const i32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

    Prefetch pf;
    prefetch<P::MINS>(pf, xq, xd, xbsum, C, T, t0, 0);
    __syncthreads();  // sbase
    const uint8_t* B0 = sb + (32 * wave + l31) * Q::SLOT;
    const uint8_t* X0 = sx + l31 * P::PITCH + (P::G32 ? 16 : 8) * h;
#pragma unroll 1
    for (int64_t j = 0; j < nsb; ++j) {
        commit<QT>(pf, sx, sbl, sbh, sxd);
        stage_packed<QT>(blocks, sbase, j, nr, sb);
        __syncthreads();
        if (j + 1 < nsb) prefetch<P::MINS>(pf, xq, xd, xbsum, C, T, t0, j + 1);

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
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t t = t0 + 32 * tt + 8 * (i >> 2) + 4 * h + (i & 3);
            if (t < T) y[t * R + r] = bf16 ? f2bf(facc[tt][i]) : f2h(facc[tt][i]);
        }
}

constexpr bool a8_type(int q) { return q == GQ_Q8_0 || (q >= GQ_Q2_K && q <= GQ_Q6_K); }

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_quantize_act_q8(const void* x, int64_t T, int64_t C, int x_dtype, int8_t* xq, float* xd, int16_t* xbsum, void* stream) {
    if (int rc = options_ok()) return rc;
    const char* who = "gq_quantize_act_q8";
    if (x_dtype != GQ_F16 && x_dtype != GQ_BF16)
        GQ_FAIL(GQ_E_BAD_TYPE, "%s: x_dtype %d (GQ_F16 or GQ_BF16; there is no fp32 path)", who, x_dtype);
    if (int rc = need(who, "x", x)) return rc;
    if (int rc = need(who, "xq", xq)) return rc;
    if (int rc = need(who, "xd", xd)) return rc;
    if (int rc = need(who, "xbsum", xbsum)) return rc;
    if (T < 1 || T > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: T=%ld (not in [1, 2^31))", who, (long)T);
    if (int rc = check_C256(who, C)) return rc;
    const int64_t nsb = T * (C / 256), n_wg = (nsb + 7) / 8;
    if (n_wg > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: T=%ld C=%ld is more than one launch takes", who, (long)T, (long)C);
    if (int rc = check_aligned(who, "x", x, 16)) return rc;
    if (int rc = check_aligned(who, "xq", xq, 16)) return rc;
    if (int rc = check_aligned(who, "xd", xd, 16)) return rc;
    if (int rc = check_aligned(who, "xbsum", xbsum, 16)) return rc;
    hipStream_t st = (hipStream_t)stream;
    dispatch_bool(x_dtype == GQ_BF16, [&](auto bf16) {
        hipLaunchKernelGGL((quantize_act_q8_kernel<decltype(bf16)::value>), dim3((unsigned)n_wg), dim3(256), 0, st,
                           static_cast<const uint16_t*>(x), nsb, xq, xd, xbsum);
    });
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

int gq_linear_packed_a8(int q_type, const void* blocks, const int32_t* row_src, int64_t R, int64_t C, const int8_t* xq,
                        const float* xd, const int16_t* xbsum, int64_t T, void* y, int y_dtype, void* stream) {
    if (int rc = options_ok()) return rc;
    const char* who = "gq_linear_packed_a8";
    if (q_type == GQ_IQ4_NL || q_type == GQ_IQ4_XS)
        GQ_FAIL(GQ_E_BAD_TYPE, "%s: q_type %d (%s) is not served on int8 activations (a K-quant or GQ_Q8_0)", who, q_type,
                q_type == GQ_IQ4_NL ? "GQ_IQ4_NL" : "GQ_IQ4_XS");
    if (!a8_type(q_type)) GQ_FAIL(GQ_E_BAD_TYPE, "%s: unknown q_type %d (a K-quant or GQ_Q8_0)", who, q_type);
    if (y_dtype != GQ_F16 && y_dtype != GQ_BF16)
        GQ_FAIL(GQ_E_BAD_TYPE, "%s: y_dtype %d (GQ_F16 or GQ_BF16; there is no fp32 path)", who, y_dtype);
    if (int rc = need(who, "blocks", blocks)) return rc;
    if (int rc = need(who, "xq", xq)) return rc;
    if (int rc = need(who, "xd", xd)) return rc;
    if (int rc = need(who, "xbsum", xbsum)) return rc;
    if (int rc = need(who, "y", y)) return rc;
    if (int rc = check_R(who, R)) return rc;
    if (T < 1 || T > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: T=%ld (not in [1, 2^31))", who, (long)T);
    if (int rc = check_C256(who, C)) return rc;
    if (int rc = check_blocks_aligned(who, q_type, blocks)) return rc;
    if (int rc = check_aligned(who, "row_src", row_src, 4)) return rc;
    if (int rc = check_aligned(who, "xq", xq, 16)) return rc;
    if (int rc = check_aligned(who, "xd", xd, 16)) return rc;
    if (int rc = check_aligned(who, "xbsum", xbsum, 16)) return rc;
    if (int rc = check_aligned(who, "y", y, 16)) return rc;
    const int64_t n_rt = (R + TR - 1) / TR, n_tt = (T + TT - 1) / TT;
    if (n_tt > 0x7fffffff / n_rt) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: R=%ld T=%ld is more than one launch takes", who, (long)R, (long)T);
    const dim3 grid((unsigned)(n_rt * n_tt));
    hipStream_t st = (hipStream_t)stream;
    dispatch_packed(q_type, [&](auto qt) {
        constexpr int QT = decltype(qt)::value;
        if constexpr (a8_type(QT))
            hipLaunchKernelGGL((linear_packed_a8_kernel<QT>), grid, dim3(256), 0, st, static_cast<const uint8_t*>(blocks), row_src, R,
                               C, xq, xd, xbsum, T, static_cast<uint16_t*>(y), (int)(y_dtype == GQ_BF16), (uint32_t)n_rt);
    });
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
