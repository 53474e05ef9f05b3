// gq_block_decode.hpp -- the device side of the block decoder (K-quants, Q8_0, IQ4_NL and IQ4_XS), shared by decode/gq_decode.hip (K15: one
// matrix per launch), search/gq_switch.hip (K18: a table of matrices per launch) and, through qgemm/gq_qgemm_core.hpp and
// qgemm/gq_gemv_core.hpp, the four packed matmul files qgemm/gq_qgemm.hip, gq_qgemv.hip, gq_moe_gemv.hip and gq_moe_gemm.hip
// (K21, K22, K24, K25: decode16 at the end, the weight operand of a GEMM / GEMV).  One text, so the entry points
// cannot drift apart: a turn of either kernel is decode_turn() (K-quants, IQ4_XS) or decode_turn_b32() (Q8_0, IQ4_NL) below.
// The host side of the same types -- the list of them, alignment, geometry, operand checks -- is gq_block_host.hpp.
// Layouts, staging widths and the numerical contract are described at the top of decode/gq_decode.hip.
#pragma once

#include "../gq_common.hpp"
#include "../../../include/gptq_gguf_iq4.h"  // (includes gptq_gguf_q8.h)

namespace gq {
namespace blockdec {

constexpr int DB = 16;  // blocks per turn: 256 threads x 16 values

template <int QT> struct Lay;
//                                  type_size, LDS slot, staging width, scale groups, offset of the stored code
template <> struct Lay<GQ_Q2_K> { static constexpr int TS = 84, TSP = 96, AL = 4, NG = 16, OFF = 0; };
template <> struct Lay<GQ_Q3_K> { static constexpr int TS = 110, TSP = 112, AL = 2, NG = 16, OFF = 4; };
template <> struct Lay<GQ_Q4_K> { static constexpr int TS = 144, TSP = 144, AL = 16, NG = 8, OFF = 0; };
template <> struct Lay<GQ_Q5_K> { static constexpr int TS = 176, TSP = 176, AL = 16, NG = 8, OFF = 0; };
template <> struct Lay<GQ_Q6_K> { static constexpr int TS = 210, TSP = 224, AL = 2, NG = 16, OFF = 32; };
// IQ4_XS { fp16 d; uint16 scales_h; uint8 scales_l[4]; uint8 qs[128]; }: 136 = 17 x 8 bytes.  The block lies at byte 8 of its
// slot, so that qs is 16-byte aligned in LDS; the stored code is kv[nibble] + 128 (iq4_code4)
template <> struct Lay<GQ_IQ4_XS> { static constexpr int TS = 136, TSP = 144, AL = 8, NG = 8, OFF = 128; };
template <int QT> constexpr int LOFF = QT == GQ_IQ4_XS ? 8 : 0;  // LDS byte of the block's first byte within its slot
constexpr int TSP_MAX = 224;  // the widest LDS slot (Q6_K)

template <int AL> struct Unit;
template <> struct Unit<2> { using T = uint16_t; };
template <> struct Unit<4> { using T = uint32_t; };
template <> struct Unit<8> { using T = uint32_t __attribute__((ext_vector_type(2))); };
template <> struct Unit<16> { using T = uint4; };

__device__ __forceinline__ uint32_t ld4(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }
__device__ __forceinline__ uint16_t ld2(const uint8_t* p) { return *reinterpret_cast<const uint16_t*>(p); }
__device__ __forceinline__ void ld16(const uint8_t* p, uint32_t w[4]) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
}

// Four IQ4 codes, one nibble per byte of n, through ggml's kvalues_iq4nl = { -127, -104, -83, -65, -49, -35, -22, -10, 1, 13,
// 25, 38, 53, 69, 89, 113 }: byte i of the result is kv[nibble i] + 128.  The table lives in four registers (constants) and is
// indexed with byte permutes: v_perm_b32 takes bytes 0-3 from its second operand and 4-7 from its first, so the low three bits
// of a nibble select within each half of the table and its bit 3 selects the half.  Six VALU operations per four values; no
// LDS or memory traffic (a per-lane index cannot use a scalar constant load).
__device__ __forceinline__ uint32_t iq4_code4(uint32_t n) {
    constexpr uint32_t KV0 = 0x3F2D1801u, KV1 = 0x766A5D4Fu, KV2 = 0xA6998D81u, KV3 = 0xF1D9C5B5u;  // kv + 128, four to a word
    const uint32_t s = n & 0x07070707u;
    const uint32_t lo = __builtin_amdgcn_perm(KV1, KV0, s), hi = __builtin_amdgcn_perm(KV3, KV2, s);
    return __builtin_amdgcn_perm(hi, lo, ((n >> 1) & 0x04040404u) | 0x03020100u);
}

// (d, dmin) bits of the block at LDS slot B
template <int QT>
__device__ __forceinline__ void block_d(const uint8_t* B, uint16_t& d, uint16_t& dmin) {
    if constexpr (QT == GQ_Q2_K) d = ld2(B + 80), dmin = ld2(B + 82);
    else if constexpr (QT == GQ_Q3_K) d = ld2(B + 108), dmin = 0;
    else if constexpr (QT == GQ_Q6_K) d = ld2(B + 208), dmin = 0;
    else if constexpr (QT == GQ_IQ4_XS) d = ld2(B + 8), dmin = 0;
    else d = ld2(B), dmin = ld2(B + 2);
}

// scale / min of group g (Q3_K / Q6_K: the signed scale, mn = 0)
template <int QT>
__device__ __forceinline__ void group_scale(const uint8_t* B, int g, int& sc, int& mn) {
    if constexpr (QT == GQ_Q2_K) {  // scales[16]: low nibble scale, high nibble min
        const uint32_t v = B[g];
        sc = v & 0xF, mn = v >> 4;
    } else if constexpr (QT == GQ_Q3_K) {  // scales[12] at 96: 16 six-bit values, low nibbles in bytes 0..7, high pairs in 8..11
        const uint32_t wl = ld4(B + 96 + 4 * ((g >> 2) & 1)), wh = ld4(B + 104);
        const uint32_t lo = (wl >> (8 * (g & 3) + 4 * (g >> 3))) & 0xF;
        const uint32_t hi = (wh >> (8 * (g & 3) + 2 * (g >> 2))) & 3;
        sc = (int)(lo | (hi << 4)) - 32, mn = 0;
    } else if constexpr (QT == GQ_Q6_K) {  // scales[16] at 192, int8
        sc = (int8_t)B[192 + g], mn = 0;
    } else if constexpr (QT == GQ_IQ4_XS) {  // scales_h at 10: two high bits per sub-block; scales_l[4] at 12: a nibble each
        const uint32_t wh = ld4(B + 8), wl = ld4(B + 12);
        sc = (int)(((wl >> (4 * g)) & 0xF) | (((wh >> (16 + 2 * g)) & 3) << 4)) - 32, mn = 0;
    } else {  // Q4_K / Q5_K: get_scale_min_k4 on the 12 bytes at 4
        const uint32_t w0 = ld4(B + 4), w1 = ld4(B + 8), w2 = ld4(B + 12);
        if (g < 4) {
            sc = (w0 >> (8 * g)) & 63, mn = (w1 >> (8 * g)) & 63;
        } else {
            const int s = 8 * (g - 4);
            sc = ((w2 >> s) & 0xF) | (((w0 >> (s + 6)) & 3) << 4);
            mn = ((w2 >> (s + 4)) & 0xF) | (((w1 >> (s + 6)) & 3) << 4);
        }
    }
}

// the 16 codes 16 g16 .. 16 g16 + 15 of the block, one per byte, as stored (Q3_K: code + 4, Q6_K: code + 32, IQ4_XS: kv + 128)
template <int QT>
__device__ __forceinline__ void codes16(const uint8_t* B, int g16, uint32_t c[4]) {
    const int l0 = (g16 & 1) * 16;
    uint32_t q[4], h[4];
    if constexpr (QT == GQ_Q2_K) {  // qs[64] at 16: 128-value chunk ch, quarter k = bits 2k, 2k+1 of byte l
        const int ch = g16 >> 3, k = (g16 >> 1) & 3;
        ld16(B + 16 + ch * 32 + l0, q);
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = (q[i] >> (2 * k)) & 0x03030303u;
    } else if constexpr (QT == GQ_Q3_K) {  // hmask[32] qs[64]: low2 | hbit << 2 (hbit set = no -4)
        const int ch = g16 >> 3, k = (g16 >> 1) & 3;
        ld16(B + 32 + ch * 32 + l0, q);
        ld16(B + l0, h);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            c[i] = ((q[i] >> (2 * k)) & 0x03030303u) | (((h[i] >> (ch * 4 + k)) & 0x01010101u) << 2);
    } else if constexpr (QT == GQ_Q4_K) {  // qs[128] at 16: 64-value chunk j, low nibbles then high nibbles
        const int j = g16 >> 2, hi = (g16 >> 1) & 1;
        ld16(B + 16 + 32 * j + l0, q);
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = (q[i] >> (4 * hi)) & 0x0f0f0f0fu;
    } else if constexpr (QT == GQ_Q5_K) {  // qh[32] at 16, qs[128] at 48: bit (2 j + hi) of qh[l] is the fifth bit
        const int j = g16 >> 2, hi = (g16 >> 1) & 1;
        ld16(B + 48 + 32 * j + l0, q);
        ld16(B + 16 + l0, h);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            c[i] = ((q[i] >> (4 * hi)) & 0x0f0f0f0fu) | (((h[i] >> (2 * j + hi)) & 0x01010101u) << 4);
    } else if constexpr (QT == GQ_IQ4_XS) {  // qs[128] at 16: sub-block ib = g16 >> 1, low nibbles then high nibbles
        ld16(B + 16 + 16 * (g16 >> 1), q);
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = iq4_code4((q[i] >> (4 * (g16 & 1))) & 0x0f0f0f0fu);
    } else {  // Q6_K ql[128] qh[64] at 128: chunk ch, quarter k: nibble (k >> 1) of ql[64 ch + 32 (k & 1) + l], bits 2k of qh
        const int ch = g16 >> 3, k = (g16 >> 1) & 3;
        ld16(B + 64 * ch + 32 * (k & 1) + l0, q);
        ld16(B + 128 + 32 * ch + l0, h);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            c[i] = ((q[i] >> (4 * (k >> 1))) & 0x0f0f0f0fu) | (((h[i] >> (2 * k)) & 0x03030303u) << 4);
    }
}

// Stage the nb blocks of a turn: ssrc[b] = index of output block b0 + b in the packed buffer, then AL-wide loads of
// exactly the blocks' bytes (all loads of a thread in flight before its first LDS write).  Ends with a barrier.
template <int QT>
__device__ __forceinline__ void stage_blocks(const uint8_t* __restrict__ blocks, const int32_t* __restrict__ row_src,
                                             int64_t b0, int nb, int64_t nbr, uint8_t* sb, int64_t* ssrc) {
    using L = Lay<QT>;
    using U = typename Unit<L::AL>::T;
    constexpr int UPB = L::TS / L::AL;                 // staging units per block
    constexpr int NIT = (DB * UPB + 255) / 256;
    const int tid = threadIdx.x;
    if (tid < nb) {
        const int64_t o = b0 + tid, r = o / nbr, j = o - r * nbr;
        ssrc[tid] = (row_src ? (int64_t)row_src[r] : r) * nbr + j;
    }
    __syncthreads();
    U v[NIT] = {};
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int u = tid + 256 * it, b = u / UPB, o = u - b * UPB;
        if (u < nb * UPB) v[it] = *reinterpret_cast<const U*>(blocks + ssrc[b] * L::TS + o * L::AL);
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int u = tid + 256 * it, b = u / UPB, o = u - b * UPB;
        if (u < nb * UPB) *reinterpret_cast<U*>(sb + b * L::TSP + LOFF<QT> + o * L::AL) = v[it];
    }
    __syncthreads();
}

template <typename OutT>
__device__ __forceinline__ OutT cvt_out(float v);
struct half_bits { uint16_t b; };
struct bf16_bits { uint16_t b; };
template <> __device__ __forceinline__ float cvt_out<float>(float v) { return v; }
template <> __device__ __forceinline__ half_bits cvt_out<half_bits>(float v) { return {f2h(v)}; }
template <> __device__ __forceinline__ bf16_bits cvt_out<bf16_bits>(float v) { return {f2bf(v)}; }

// One turn of a workgroup of 256 threads: output blocks b0 .. b0 + nb - 1 (nb <= DB) of a matrix with nbr blocks per row,
// staged in sb (DB * Lay<QT>::TSP bytes, 16-byte aligned) and decoded to out + b0 * 256.  The caller puts a barrier
// between two turns that use the same sb / ssrc.
template <int QT, typename OutT>
__device__ __forceinline__ void decode_turn(const uint8_t* __restrict__ blocks, const int32_t* __restrict__ row_src,
                                            int64_t b0, int nb, int64_t nbr, OutT* __restrict__ out, uint8_t* sb,
                                            int64_t* ssrc) {
    using L = Lay<QT>;
    const int tid = threadIdx.x, b = tid >> 4, g16 = tid & 15;
    stage_blocks<QT>(blocks, row_src, b0, nb, nbr, sb, ssrc);
    if (b < nb) {
        const uint8_t* B = sb + b * L::TSP;
        uint16_t d, dmin;
        int sc, mn;
        block_d<QT>(B, d, dmin);
        group_scale<QT>(B, g16 * L::NG / 16, sc, mn);
        const float ds = h2f(d) * (float)sc, dm = h2f(dmin) * (float)mn;
        uint32_t c[4];
        codes16<QT>(B, g16, c);
        alignas(16) OutT o[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float code = (float)((c[k >> 2] >> (8 * (k & 3))) & 0xffu) - (float)L::OFF;
            o[k] = cvt_out<OutT>(dequantize1(code, ds, dm));
        }
        uint4* op = reinterpret_cast<uint4*>(out + (b0 + b) * 256 + 16 * g16);
#pragma unroll
        for (int k = 0; k < (int)sizeof(OutT) * 16 / 16; ++k) op[k] = reinterpret_cast<const uint4*>(o)[k];
    }
}

// ---- the 32-value types.  Q8_0: block_q8_0 { fp16 d; int8 qs[32]; }, 34 bytes; IQ4_NL: block_iq4_nl { fp16 d; uint8 qs[16]; },
// 18 bytes; both 2-byte aligned.  A turn is B32_DB = 128 consecutive output blocks -- the 4096 values of a K-quant turn -- and a
// thread produces half a block.  Block b of the turn lies in the LDS slot of B32_SLOT = 48 bytes at sb + 48 b with d at byte 14
// and the code bytes from byte 16 on: staging unit u (2 bytes, u = 0 .. 16 / 0 .. 8) of a block goes to byte 14 + 2 u, so that
// each half of Q8_0's codes, and all of IQ4_NL's, is one aligned 16-byte LDS read.
template <int QT> struct Lay32;
template <> struct Lay32<GQ_Q8_0> { static constexpr int TS = 34, UPB = 17; };
template <> struct Lay32<GQ_IQ4_NL> { static constexpr int TS = 18, UPB = 9; };
constexpr int B32_DB = 128, B32_SLOT = 48;
constexpr int Q8_TS = Lay32<GQ_Q8_0>::TS, Q8_UPB = Lay32<GQ_Q8_0>::UPB;
constexpr int NL_TS = Lay32<GQ_IQ4_NL>::TS, NL_UPB = Lay32<GQ_IQ4_NL>::UPB;
constexpr int SB_BYTES = B32_DB * B32_SLOT > DB * TSP_MAX ? B32_DB * B32_SLOT : DB * TSP_MAX;  // LDS of a kernel that takes any turn
constexpr int SSRC_N = B32_DB > DB ? B32_DB : DB;

// one value: the stored byte as int8, times d -- exact in fp32 (shared with qgemm/gq_qgemm.hip)
__device__ __forceinline__ float q8_0_dequantize1(float d, uint32_t byte) { return d * (float)(int8_t)byte; }
// one value of IQ4_NL: byte = kv + 128 (iq4_code4); the difference and the product are exact in fp32
__device__ __forceinline__ float iq4_nl_dequantize1(float d, uint32_t byte) { return d * ((float)byte - 128.f); }

// the 16 values of half h of the 32-value block whose d is at `pd` and whose code bytes start at `pc` (16-byte aligned)
template <int QT, typename OutT>
__device__ __forceinline__ void decode_half32(const uint8_t* pd, const uint8_t* pc, int h, OutT o[16]) {
    const float d = h2f(ld2(pd));
    uint32_t c[4];
    if constexpr (QT == GQ_Q8_0) {
        ld16(pc + 16 * h, c);
#pragma unroll
        for (int k = 0; k < 16; ++k) o[k] = cvt_out<OutT>(q8_0_dequantize1(d, (c[k >> 2] >> (8 * (k & 3))) & 0xffu));
    } else {  // IQ4_NL: the low nibbles of qs[0 .. 15] are values 0 .. 15, the high nibbles 16 .. 31
        ld16(pc, c);
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = iq4_code4((c[i] >> (4 * h)) & 0x0f0f0f0fu);
#pragma unroll
        for (int k = 0; k < 16; ++k) o[k] = cvt_out<OutT>(iq4_nl_dequantize1(d, (c[k >> 2] >> (8 * (k & 3))) & 0xffu));
    }
}

// One turn of a workgroup of 256 threads: output blocks b0 .. b0 + nb - 1 (nb <= B32_DB) of a matrix with nbr = C / 32 blocks
// per row, decoded to out + b0 * 32: w = f32(d) * f32(q) (IQ4_NL: f32(kv[q])), one cast.  Output block L comes from packed block
// row_src[L / nbr] * nbr + L % nbr; a turn may straddle rows.  sb: B32_DB * B32_SLOT bytes, 16-byte aligned; ssrc: B32_DB
// entries.  The caller puts a barrier between two turns that use the same sb / ssrc.
template <int QT, typename OutT>
__device__ __forceinline__ void decode_turn_b32(const uint8_t* __restrict__ blocks, const int32_t* __restrict__ row_src,
                                                int64_t b0, int nb, int64_t nbr, OutT* __restrict__ out, uint8_t* sb,
                                                int64_t* ssrc) {
    constexpr int TS = Lay32<QT>::TS, UPB = Lay32<QT>::UPB, NIT = (B32_DB * UPB + 255) / 256;
    const int tid = threadIdx.x;
    if (tid < nb) {
        const int64_t o = b0 + tid, r = o / nbr, j = o - r * nbr;
        ssrc[tid] = (row_src ? (int64_t)row_src[r] : r) * nbr + j;
    }
    __syncthreads();
    uint16_t v[NIT] = {};
#pragma unroll
    for (int it = 0; it < NIT; ++it) {  // 2-byte loads of exactly the blocks' bytes, all in flight before the first LDS write
        const int u = tid + 256 * it, b = u / UPB, o = u - b * UPB;
        if (u < nb * UPB) v[it] = ld2(blocks + ssrc[b] * TS + o * 2);
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int u = tid + 256 * it, b = u / UPB, o = u - b * UPB;
        if (u < nb * UPB) *reinterpret_cast<uint16_t*>(sb + b * B32_SLOT + 14 + o * 2) = v[it];
    }
    __syncthreads();
    const int b = tid >> 1, h = tid & 1;
    if (b < nb) {
        const uint8_t* B = sb + b * B32_SLOT;
        alignas(16) OutT o[16];
        decode_half32<QT, OutT>(B + 14, B + 16, h, o);
        uint4* op = reinterpret_cast<uint4*>(out + (b0 + b) * 32 + 16 * h);
#pragma unroll
        for (int k = 0; k < (int)sizeof(OutT) * 16 / 16; ++k) op[k] = reinterpret_cast<const uint4*>(o)[k];
    }
}

// ---- the packed weight as a GEMM / GEMV operand (qgemm/gq_qgemm.hip K21, qgemm/gq_qgemv.hip K22): a row's share of one
// superblock of 256 values lies in an LDS slot of its own and a lane decodes 16 consecutive values of it.
// the staging of one row's share of a superblock: UPR units of AL bytes, unit o at LDS byte lds_off(o) of the row's slot
template <int QT> struct QL {
    using L = Lay<QT>;
    static constexpr int AL = L::AL, UPR = L::TS / L::AL, ROWB = L::TS;
    static constexpr int SLOT = ((L::TS + 15) / 16 | 1) * 16;
    static __device__ __forceinline__ int lds_off(int o) { return LOFF<QT> + o * AL; }
};
template <> struct QL<GQ_Q8_0> {  // 8 blocks of 34 bytes: the eight d at bytes 0 .. 15, block b's 32 codes at 16 + 32 b
    static constexpr int AL = 2, UPR = 8 * Q8_UPB, ROWB = 8 * Q8_TS;
    static constexpr int SLOT = 16 + 8 * 32 + 32;
    static __device__ __forceinline__ int lds_off(int o) {
        const int b = o / Q8_UPB, w = o - b * Q8_UPB;
        return w == 0 ? 2 * b : 16 + 32 * b + 2 * (w - 1);
    }
};
template <> struct QL<GQ_IQ4_NL> {  // 8 blocks of 18 bytes: the eight d at bytes 0 .. 15, block b's 16 code bytes at 16 + 16 b
    static constexpr int AL = 2, UPR = 8 * NL_UPB, ROWB = 8 * NL_TS;
    static constexpr int SLOT = 16 + 8 * 16;
    static __device__ __forceinline__ int lds_off(int o) {
        const int b = o / NL_UPB, w = o - b * NL_UPB;
        return w == 0 ? 2 * b : 16 + 16 * b + 2 * (w - 1);
    }
};
static_assert(QL<GQ_Q8_0>::SLOT / 16 % 2 == 1 && QL<GQ_IQ4_NL>::SLOT / 16 % 2 == 1 && QL<GQ_IQ4_XS>::SLOT / 16 % 2 == 1,
              "an odd number of 16-byte units");
static_assert(QL<GQ_IQ4_XS>::SLOT == Lay<GQ_IQ4_XS>::TSP && LOFF<GQ_IQ4_XS> + Lay<GQ_IQ4_XS>::TS <= QL<GQ_IQ4_XS>::SLOT, "the block fits its slot");

// The 16 values 64 c + 16 q .. + 15 of the superblock in slot B, as 8 words of two OutT bit patterns: decode_turn's text.
template <int QT, typename OutT>
__device__ __forceinline__ void decode16(const uint8_t* B, int c, int q, uint32_t w[8]) {
    uint16_t o[16];
    if constexpr (QT == GQ_Q8_0 || QT == GQ_IQ4_NL) {
        const int b = 2 * c + (q >> 1);
        OutT v[16];
        decode_half32<QT, OutT>(B + 2 * b, B + 16 + (QT == GQ_Q8_0 ? 32 : 16) * b, q & 1, v);
#pragma unroll
        for (int k = 0; k < 16; ++k) o[k] = v[k].b;
    } else {
        using L = Lay<QT>;
        uint32_t cd[4];
        const int g16 = 4 * c + q;
        uint16_t d, dmin;
        int sc, mn;
        block_d<QT>(B, d, dmin);
        group_scale<QT>(B, g16 * L::NG / 16, sc, mn);
        const float ds = h2f(d) * (float)sc, dm = h2f(dmin) * (float)mn;
        codes16<QT>(B, g16, cd);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float code = (float)((cd[k >> 2] >> (8 * (k & 3))) & 0xffu) - (float)L::OFF;
            o[k] = cvt_out<OutT>(dequantize1(code, ds, dm)).b;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = (uint32_t)o[2 * k] | ((uint32_t)o[2 * k + 1] << 16);
}

}  // namespace blockdec
}  // namespace gq
