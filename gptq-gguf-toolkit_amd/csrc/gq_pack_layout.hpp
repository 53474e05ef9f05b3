// gq_pack_layout.hpp -- the five K-quant block layouts as "output dword w of a block" (reference packing_utils.py:8-326), and
// the turn that assembles PB staged blocks and stores them: shared by gq_pack's kernel (gq_codec.hip) and gq_pack_bands'
// (levels/gq_levelpack.hip), so that both write the same bytes from one text.
#pragma once
#include "gq_common.hpp"

namespace gq {

constexpr int PB = 32;  // 256-value blocks a workgroup packs per turn

__device__ __forceinline__ uint8_t pack_scale_min_byte(const uint8_t* sc, const uint8_t* mn, int j) {
    // packing_utils.py:8-30, byte j of the 12
    if (j < 4) return (uint8_t)(sc[j] | ((sc[4 + j] >> 4) << 6));
    if (j < 8) return (uint8_t)(mn[j - 4] | ((mn[j] >> 4) << 6));
    return (uint8_t)((sc[j - 4] & 0x0F) | ((mn[j - 4] & 0x0F) << 4));
}

template <int QT>
__device__ __forceinline__ uint8_t pack_byte(const uint8_t* q, const uint8_t* sb, const uint8_t* mb, uint16_t d,
                                             uint16_t dmin, int o) {
    if constexpr (QT == GQ_Q2_K) {  // :33-77  scales[16] qs[64] d dmin
        if (o < 16) return (uint8_t)((sb[o] & 0x0F) | ((mb[o] & 0x0F) << 4));
        if (o < 80) {
            int t = o - 16, ch = t >> 5, l = t & 31;
            const uint8_t* c = q + ch * 128;
            return (uint8_t)(c[l] | (c[32 + l] << 2) | (c[64 + l] << 4) | (c[96 + l] << 6));
        }
        if (o < 82) return (uint8_t)(d >> (8 * (o - 80)));
        return (uint8_t)(dmin >> (8 * (o - 82)));
    } else if constexpr (QT == GQ_Q3_K) {  // :80-142  hmask[32] qs[64] scales[12] d
        if (o < 32) {
            uint8_t h = 0;
#pragma unroll
            for (int b = 0; b < 8; ++b) h |= (uint8_t)(((uint8_t)((int8_t)q[b * 32 + o] + 4) > 3) << b);
            return h;
        }
        if (o < 96) {
            int t = o - 32, ch = t >> 5, l = t & 31;
            const uint8_t* c = q + ch * 128;
            uint8_t v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint8_t u = (uint8_t)((int8_t)c[32 * k + l] + 4);
                v[k] = u > 3 ? (uint8_t)(u - 4) : u;
            }
            return (uint8_t)(v[0] | (v[1] << 2) | (v[2] << 4) | (v[3] << 6));
        }
        if (o < 108) {
            int j = o - 96;  // :103-115
            auto sc = [&](int k) { return (uint8_t)((int8_t)sb[k] + 32); };
            if (j < 8) return (uint8_t)((sc(j) & 0x0F) | ((sc(j + 8) & 0x0F) << 4));
            int t = j - 8;
            return (uint8_t)(((sc(t) >> 4) & 3) | (((sc(t + 4) >> 4) & 3) << 2) | (((sc(t + 8) >> 4) & 3) << 4) |
                             (((sc(t + 12) >> 4) & 3) << 6));
        }
        return (uint8_t)(d >> (8 * (o - 108)));
    } else if constexpr (QT == GQ_Q4_K) {  // :145-190  d dmin scales[12] qs[128]
        if (o < 2) return (uint8_t)(d >> (8 * o));
        if (o < 4) return (uint8_t)(dmin >> (8 * (o - 2)));
        if (o < 16) return pack_scale_min_byte(sb, mb, o - 4);
        int t = o - 16, base = (t >> 5) * 64, l = t & 31;
        return (uint8_t)(q[base + l] | (q[base + 32 + l] << 4));
    } else if constexpr (QT == GQ_Q5_K) {  // :193-262  d dmin scales[12] qh[32] ql[128]
        if (o < 2) return (uint8_t)(d >> (8 * o));
        if (o < 4) return (uint8_t)(dmin >> (8 * (o - 2)));
        if (o < 16) return pack_scale_min_byte(sb, mb, o - 4);
        if (o < 48) {
            int j = o - 16;
            uint8_t h = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                h |= (uint8_t)((q[64 * k + j] > 15) << (2 * k));
                h |= (uint8_t)((q[64 * k + 32 + j] > 15) << (2 * k + 1));
            }
            return h;
        }
        int t = o - 48, base = (t >> 5) * 64, j = t & 31;
        return (uint8_t)((q[base + j] & 15) | ((q[base + 32 + j] & 15) << 4));
    } else {  // Q6_K :265-326  ql[128] qh[64] scales[16] d
        auto v = [&](int idx) { return (uint8_t)((int8_t)q[idx] + 32); };
        if (o < 128) {
            int ch = o >> 6, t = o & 63, l = t & 31, hi = t >> 5;
            int b = ch * 128 + l + 32 * hi;
            return (uint8_t)((v(b) & 0xF) | ((v(b + 64) & 0xF) << 4));
        }
        if (o < 192) {
            int t = o - 128, ch = t >> 5, l = t & 31, b = ch * 128 + l;
            return (uint8_t)(((v(b) >> 4) & 3) | (((v(b + 32) >> 4) & 3) << 2) | (((v(b + 64) >> 4) & 3) << 4) |
                             (((v(b + 96) >> 4) & 3) << 6));
        }
        if (o < 208) return sb[o - 192];
        return (uint8_t)(d >> (8 * (o - 208)));
    }
}

// ---- four output bytes at a time ----
// Every field of every block layout starts at a multiple of 4 bytes (only the trailing fp16 `d` of Q3_K / Q6_K is a
// 2-byte tail), and the strides the layouts combine (32, 64, 96, 128 input bytes) are multiples of 4 as well: output
// dword w of a block is a handful of LDS dword reads and byte-parallel mask / shift / or operations.
__device__ __forceinline__ uint32_t ld4(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }
// four independent byte additions (no carry across bytes)
__device__ __forceinline__ uint32_t add4(uint32_t x, uint32_t c) {
    return ((x & 0x7f7f7f7fu) + (c & 0x7f7f7f7fu)) ^ ((x ^ c) & 0x80808080u);
}
template <int QT>
__device__ __forceinline__ uint32_t pack_dword(const uint8_t* q, const uint8_t* sb, const uint8_t* mb, uint16_t d,
                                               uint16_t dmin, int w) {
    const int o = 4 * w;
    auto hdr = [&](int j0) {  // four bytes of the 12-byte scale/min field of Q4_K / Q5_K
        return (uint32_t)pack_scale_min_byte(sb, mb, j0) | ((uint32_t)pack_scale_min_byte(sb, mb, j0 + 1) << 8) |
               ((uint32_t)pack_scale_min_byte(sb, mb, j0 + 2) << 16) | ((uint32_t)pack_scale_min_byte(sb, mb, j0 + 3) << 24);
    };
    if constexpr (QT == GQ_Q2_K) {  // scales[16] qs[64] d dmin
        if (o < 16) return (ld4(sb + o) & 0x0f0f0f0fu) | ((ld4(mb + o) & 0x0f0f0f0fu) << 4);
        if (o < 80) {
            const int t = o - 16, ch = t >> 5, l = t & 31;
            const uint8_t* c = q + ch * 128 + l;
            return ld4(c) | (ld4(c + 32) << 2) | (ld4(c + 64) << 4) | (ld4(c + 96) << 6);  // values 0..3: no masks
        }
        return (uint32_t)d | ((uint32_t)dmin << 16);
    } else if constexpr (QT == GQ_Q3_K) {  // hmask[32] qs[64] scales[12] | d
        if (o < 32) {
            uint32_t h = 0;
#pragma unroll
            for (int b = 0; b < 8; ++b) h |= ((add4(ld4(q + b * 32 + o), 0x04040404u) >> 2) & 0x01010101u) << b;  // (q+4) > 3
            return h;
        }
        if (o < 96) {
            const int t = o - 32, ch = t >> 5, l = t & 31;
            const uint8_t* c = q + ch * 128 + l;
            uint32_t r = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) r |= (add4(ld4(c + 32 * k), 0x04040404u) & 0x03030303u) << (2 * k);  // u > 3 ? u - 4 : u
            return r;
        }
        uint32_t r = 0;  // the 12 scale bytes: byte-wise (o = 96, 100, 104)
#pragma unroll
        for (int k = 0; k < 4; ++k) r |= (uint32_t)pack_byte<QT>(q, sb, mb, d, dmin, o + k) << (8 * k);
        return r;
    } else if constexpr (QT == GQ_Q4_K) {  // d dmin scales[12] qs[128]
        if (o == 0) return (uint32_t)d | ((uint32_t)dmin << 16);
        if (o < 16) return hdr(o - 4);
        const int t = o - 16, base = (t >> 5) * 64, l = t & 31;
        return ld4(q + base + l) | (ld4(q + base + 32 + l) << 4);  // values 0..15
    } else if constexpr (QT == GQ_Q5_K) {  // d dmin scales[12] qh[32] ql[128]
        if (o == 0) return (uint32_t)d | ((uint32_t)dmin << 16);
        if (o < 16) return hdr(o - 4);
        if (o < 48) {
            const int j = o - 16;
            uint32_t h = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                h |= ((ld4(q + 64 * k + j) >> 4) & 0x01010101u) << (2 * k);           // values 0..31: > 15 is bit 4
                h |= ((ld4(q + 64 * k + 32 + j) >> 4) & 0x01010101u) << (2 * k + 1);
            }
            return h;
        }
        const int t = o - 48, base = (t >> 5) * 64, j = t & 31;
        return (ld4(q + base + j) & 0x0f0f0f0fu) | ((ld4(q + base + 32 + j) & 0x0f0f0f0fu) << 4);
    } else {  // Q6_K  ql[128] qh[64] scales[16] | d ;  v = q + 32 in 0..63
        auto v4 = [&](int idx) { return add4(ld4(q + idx), 0x20202020u); };
        if (o < 128) {
            const int ch = o >> 6, t = o & 63, l = t & 31, hi = t >> 5, b = ch * 128 + l + 32 * hi;
            return (v4(b) & 0x0f0f0f0fu) | ((v4(b + 64) & 0x0f0f0f0fu) << 4);
        }
        if (o < 192) {
            const int t = o - 128, ch = t >> 5, l = t & 31, b = ch * 128 + l;
            return ((v4(b) >> 4) & 0x03030303u) | (((v4(b + 32) >> 4) & 0x03030303u) << 2) |
                   (((v4(b + 64) >> 4) & 0x03030303u) << 4) | (((v4(b + 96) >> 4) & 0x03030303u) << 6);
        }
        return ld4(sb + (o - 192));
    }
}

// ---- one turn's output ----
// nb <= PB blocks are staged in LDS (sq: 256 codes per block, ss / sm: NG group scales / mins per block, sd / sdm: the fp16 bit
// patterns) and the caller has synchronised.  Assembles the nb * TS output bytes and stores them from `op` on, which is 16-byte
// aligned (the first block of a turn is a multiple of 8 blocks into a 16-byte aligned buffer, and 8 * TS % 16 == 0).  `so` is the
// LDS image of the output for the 110- / 210-byte layouts (unused for the others).  The caller synchronises before it restages.
template <int QT, int TS, int NG>
__device__ __forceinline__ void pack_store(const uint8_t* sq, uint8_t* so, const uint8_t* ss, const uint8_t* sm,
                                           const uint16_t* sd, const uint16_t* sdm, int nb, uint8_t* __restrict__ op) {
    const int tid = threadIdx.x;
    constexpr int NDW = TS / 4;  // whole dwords of a block; TS % 4 == 2 (Q3_K, Q6_K): the fp16 d follows
    if constexpr (TS % 4 == 0) {
        // r05: 84- / 144- / 176-byte blocks are whole dwords and the workgroup's output region is contiguous: thread i's
        // dword IS output dword i -- stored straight to global memory (coalesced 4-byte stores), no LDS image of the
        // output, one barrier and one pass fewer
        uint32_t* op32 = reinterpret_cast<uint32_t*>(op);
        if constexpr (QT == GQ_Q4_K || QT == GQ_Q5_K) {
            // the 4 header dwords of a block (d | dmin, 12 scale / min bytes assembled byte by byte) take a long path:
            // in one index space every wave carries a few of them and all its lanes wait -- body dwords first (one
            // uniform path), the headers in a pass of their own
            constexpr int HD = 4, BD = NDW - HD;
            for (int i = tid; i < nb * BD; i += 256) {
                const int b = i / BD, w = HD + i % BD;
                op32[b * NDW + w] = pack_dword<QT>(sq + b * 256, ss + b * NG, sm + b * NG, sd[b], sdm[b], w);
            }
            for (int i = tid; i < nb * HD; i += 256) {
                const int b = i / HD, w = i % HD;
                op32[b * NDW + w] = pack_dword<QT>(sq + b * 256, ss + b * NG, sm + b * NG, sd[b], sdm[b], w);
            }
        } else {
            for (int i = tid; i < nb * NDW; i += 256) {
                const int b = i / NDW, w = i % NDW;
                op32[i] = pack_dword<QT>(sq + b * 256, ss + b * NG, sm + b * NG, sd[b], sdm[b], w);
            }
        }
        return;
    }
    // (r05) one pass per KIND of dword -- Q3_K: hmask 8 | qs 16 | scales 3 (byte-wise); Q6_K: ql 32 | qh 16 | scales 4 -- so that
    // every wave runs one code path (in one index space each wave carried all kinds and its lanes waited for the longest)
    constexpr int W1 = QT == GQ_Q3_K ? 8 : (QT == GQ_Q6_K ? 32 : NDW), W2 = QT == GQ_Q3_K ? 24 : (QT == GQ_Q6_K ? 48 : NDW);
    auto pass = [&](int w0, int w1) {
        const int nw = w1 - w0;
        for (int i = tid; i < nb * nw; i += 256) {
            const int b = i / nw, w = w0 + i % nw;
            const uint32_t v = pack_dword<QT>(sq + b * 256, ss + b * NG, sm + b * NG, sd[b], sdm[b], w);
            uint8_t* dst = so + b * TS + 4 * w;
            if ((TS % 4 == 0) || !(b & 1)) {
                *reinterpret_cast<uint32_t*>(dst) = v;
            } else {  // odd block of a 110- / 210-byte layout: 2-byte aligned
                reinterpret_cast<uint16_t*>(dst)[0] = (uint16_t)v;
                reinterpret_cast<uint16_t*>(dst)[1] = (uint16_t)(v >> 16);
            }
        }
    };
    pass(0, W1);
    if constexpr (W1 < NDW) pass(W1, W2);
    if constexpr (W2 < NDW) pass(W2, NDW);
    if constexpr (TS % 4 != 0) {
        if (tid < nb) *reinterpret_cast<uint16_t*>(so + tid * TS + 4 * NDW) = sd[tid];
    }
    __syncthreads();
    const int nbytes = nb * TS;
    for (int v = tid; v < nbytes / 16; v += 256)
        reinterpret_cast<uint4*>(op)[v] = reinterpret_cast<const uint4*>(so)[v];
    for (int t = (nbytes / 16) * 16 + tid; t < nbytes; t += 256) op[t] = so[t];
}

}  // namespace gq
