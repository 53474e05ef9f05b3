// gq_switch_units.hpp -- one work unit of a level switch, shared by search/gq_switch.hip (gq_level_switch: a job is one
// [R, C] matrix) and search/gq_switch_experts.hip (gq_level_switch_experts: a job is E such matrices): the SAME text, so
// the same bits.  A unit is one turn of the block decoder (blockdec::decode_turn / decode_turn_b32) or, for a dense source,
// DENSE_CHUNKS 16-byte output chunks.  `Job` is any struct with the members
//     const uint8_t* src;  uint8_t* dst;  const int32_t* row_src;  int64_t n;  int32_t per_row;  int32_t-like out_dtype;
// n: packed: blocks of the matrix (R * C / 256; Q8_0 / IQ4_NL: R * C / 32); dense: 16-byte output chunks (R * cpr);
// per_row: packed: blocks per row; dense: chunks per row (cpr).  Device code only.
#pragma once
#include "gq_block_decode.hpp"

namespace gq {
namespace switchunit {

using namespace blockdec;

constexpr int DENSE_CHUNKS = 512;  // 16-byte output chunks per dense unit (two per thread)

template <int QT, class Job>
__device__ __forceinline__ void packed_unit(const Job& J, int64_t b0, uint8_t* sb, int64_t* ssrc) {
    const int nb = (int)((J.n - b0) < DB ? (J.n - b0) : DB);
    switch (J.out_dtype) {
    case GQ_F32: decode_turn<QT, float>(J.src, J.row_src, b0, nb, J.per_row, reinterpret_cast<float*>(J.dst), sb, ssrc); break;
    case GQ_F16: decode_turn<QT, half_bits>(J.src, J.row_src, b0, nb, J.per_row, reinterpret_cast<half_bits*>(J.dst), sb, ssrc); break;
    default: decode_turn<QT, bf16_bits>(J.src, J.row_src, b0, nb, J.per_row, reinterpret_cast<bf16_bits*>(J.dst), sb, ssrc); break;
    }
}

template <int QT, class Job>
__device__ __forceinline__ void b32_unit(const Job& J, int64_t b0, uint8_t* sb, int64_t* ssrc) {
    const int nb = (int)((J.n - b0) < B32_DB ? (J.n - b0) : B32_DB);
    switch (J.out_dtype) {
    case GQ_F32: decode_turn_b32<QT, float>(J.src, J.row_src, b0, nb, J.per_row, reinterpret_cast<float*>(J.dst), sb, ssrc); break;
    case GQ_F16: decode_turn_b32<QT, half_bits>(J.src, J.row_src, b0, nb, J.per_row, reinterpret_cast<half_bits*>(J.dst), sb, ssrc); break;
    default: decode_turn_b32<QT, bf16_bits>(J.src, J.row_src, b0, nb, J.per_row, reinterpret_cast<bf16_bits*>(J.dst), sb, ssrc); break;
    }
}

template <int DT> __device__ __forceinline__ float widen(uint32_t bits);
template <> __device__ __forceinline__ float widen<GQ_F32>(uint32_t bits) { return __builtin_bit_cast(float, bits); }
template <> __device__ __forceinline__ float widen<GQ_F16>(uint32_t bits) { return h2f((uint16_t)bits); }
template <> __device__ __forceinline__ float widen<GQ_BF16>(uint32_t bits) { return bf2f((uint16_t)bits); }

// chunk k of a dense job: CH = 16 / sizeof(dst element) consecutive elements of one row
template <int SD, int OD, class Job>
__device__ __forceinline__ void dense_unit(const Job& J, int64_t k0) {
    constexpr int SES = SD == GQ_F32 ? 4 : 2, DES = OD == GQ_F32 ? 4 : 2, CH = 16 / DES, NW = CH * SES / 4;
#pragma unroll
    for (int i = 0; i < DENSE_CHUNKS / 256; ++i) {
        const int64_t k = k0 + i * 256 + threadIdx.x;
        if (k < J.n) {
            const int64_t r = k / J.per_row, cc = k - r * J.per_row;
            const int64_t sr = J.row_src ? (int64_t)J.row_src[r] : r;
            const uint8_t* sp = J.src + (sr * J.per_row + cc) * (CH * SES);
            uint32_t w[NW];
            if constexpr (NW == 2) {
                const uint2 v = *reinterpret_cast<const uint2*>(sp);
                w[0] = v.x, w[1] = v.y;
            } else {
#pragma unroll
                for (int q = 0; q < NW / 4; ++q) {
                    const uint4 v = reinterpret_cast<const uint4*>(sp)[q];
                    w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
                }
            }
            uint32_t o[4];
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                const float f = SES == 4 ? widen<SD>(w[e]) : widen<SD>((w[e >> 1] >> (16 * (e & 1))) & 0xffffu);
                if constexpr (OD == GQ_F32) o[e] = __builtin_bit_cast(uint32_t, f);
                else {
                    const uint32_t h = OD == GQ_F16 ? f2h(f) : f2bf(f);
                    o[e >> 1] = (e & 1) ? (o[e >> 1] | (h << 16)) : h;
                }
            }
            *reinterpret_cast<uint4*>(J.dst + k * 16) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
}

template <int SD, class Job>
__device__ __forceinline__ void dense_unit_from(const Job& J, int64_t k0) {
    switch (J.out_dtype) {
    case GQ_F32: dense_unit<SD, GQ_F32>(J, k0); break;
    case GQ_F16: dense_unit<SD, GQ_F16>(J, k0); break;
    default: dense_unit<SD, GQ_BF16>(J, k0); break;
    }
}

// the unit `ul` of a job of `kind`: a switch on block-uniform values, a workgroup executes one arm
template <class Job>
__device__ __forceinline__ void run_unit(const Job& J, int kind, int64_t ul, uint8_t* sb, int64_t* ssrc) {
    switch (kind) {
    case GQ_Q2_K: packed_unit<GQ_Q2_K>(J, ul * DB, sb, ssrc); break;
    case GQ_Q3_K: packed_unit<GQ_Q3_K>(J, ul * DB, sb, ssrc); break;
    case GQ_Q4_K: packed_unit<GQ_Q4_K>(J, ul * DB, sb, ssrc); break;
    case GQ_Q5_K: packed_unit<GQ_Q5_K>(J, ul * DB, sb, ssrc); break;
    case GQ_Q6_K: packed_unit<GQ_Q6_K>(J, ul * DB, sb, ssrc); break;
    case GQ_IQ4_XS: packed_unit<GQ_IQ4_XS>(J, ul * DB, sb, ssrc); break;
    case GQ_Q8_0: b32_unit<GQ_Q8_0>(J, ul * B32_DB, sb, ssrc); break;
    case GQ_IQ4_NL: b32_unit<GQ_IQ4_NL>(J, ul * B32_DB, sb, ssrc); break;
    case GQ_F32: dense_unit_from<GQ_F32>(J, ul * DENSE_CHUNKS); break;
    case GQ_F16: dense_unit_from<GQ_F16>(J, ul * DENSE_CHUNKS); break;
    default: dense_unit_from<GQ_BF16>(J, ul * DENSE_CHUNKS); break;
    }
}

}  // namespace switchunit
}  // namespace gq
