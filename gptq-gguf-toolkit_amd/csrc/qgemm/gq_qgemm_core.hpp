// gq_qgemm_core.hpp -- the one text of the packed tile GEMM: staging, K loop and epilogue of a workgroup of 4 waves that owns
// an output tile of TR = 128 weight rows and TT tokens.  gq_qgemm.hip (K21: tile token i = token t0 + i of x and of y) and
// gq_moe_gemm.hip (K25: tile token i = the i-th pair of an expert's run, its x row gathered and its y row scattered through
// `order`) include it, so for one weight row and one input row the two kernels run the same instructions in the same order:
// superblock j, chunk c, step s, 32 k per MFMA, into an accumulator no other token touches -- the same bits.  The form is
// described at the head of gq_qgemm.hip.
// Device code only: the entry points' type dispatch and operand checks are search/gq_block_host.hpp's.
#pragma once
#include <type_traits>

#include "../search/gq_block_decode.hpp"

namespace gq {
namespace gemmcore {

using namespace blockdec;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int TR = 128, KC = 64;  // tile of rows; k of an x chunk (the token tile TT = 256 or 128 is a template parameter)
constexpr int64_t WIDE_TILES = 512;  // two workgroups on each of the 256 CUs: from there on the 256-token tile is used

// a row of x or of y that a tile token stands for; !on: the tile has no such token (x reads as zeros, y is not stored)
struct Row {
    bool on;
    int64_t row;
};

// Stage superblock j of the tile's nr rows: sbase[r] = byte offset of the row's first block.  The caller has a barrier before
// (sb free) and after.
template <int QT>
__device__ __forceinline__ void stage_rows(const uint8_t* __restrict__ blocks, const int64_t* sbase, int64_t j, int nr,
                                           uint8_t* sb) {
    using Q = QL<QT>;
    using U = typename Unit<Q::AL>::T;
    constexpr int NIT = (TR * Q::UPR + 255) / 256, GRP = 8;
    const int tid = threadIdx.x, n = nr * Q::UPR;
#pragma unroll 1
    for (int it0 = 0; it0 < NIT; it0 += GRP) {
        if (tid + 256 * it0 >= n) break;
        U v[GRP] = {};
#pragma unroll
        for (int g = 0; g < GRP; ++g) {
            const int u = tid + 256 * (it0 + g), r = u / Q::UPR, o = u - r * Q::UPR;
            if (u < n) v[g] = *reinterpret_cast<const U*>(blocks + sbase[r] + j * Q::ROWB + o * Q::AL);
        }
#pragma unroll
        for (int g = 0; g < GRP; ++g) {
            const int u = tid + 256 * (it0 + g), r = u / Q::UPR, o = u - r * Q::UPR;
            if (u < n) *reinterpret_cast<U*>(sb + r * Q::SLOT + Q::lds_off(o)) = v[g];
        }
    }
}

template <bool BF16>
__device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
    if constexpr (BF16)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// the XP 16-byte pieces of a thread of x chunk (k0 .. k0 + 63) of the tile's TT tokens: piece p = tid + 256 i is tile token
// p >> 3, 8-k piece p & 7 (a token's 128 bytes are read by 8 consecutive lanes); xrow(i) is that token's row of x
template <int XP, class XRow>
__device__ __forceinline__ void load_x(const uint8_t* __restrict__ x, int64_t C, int64_t k0, XRow xrow, u32x4 xr[XP]) {
#pragma unroll
    for (int i = 0; i < XP; ++i) {
        const int p = threadIdx.x + 256 * i;
        const Row t = xrow(i);
        xr[i] = t.on ? *reinterpret_cast<const u32x4*>(x + (t.row * C + k0 + 8 * (p & 7)) * 2) : u32x4{0, 0, 0, 0};
    }
}

// The tile [TT tokens, rows r0 .. r0 + nr - 1]: y[yrow(tt)][r] = sum_c W[r][c] x[xrow(i)][c].  sbase[r] (LDS, written by the
// caller; the first barrier here publishes it) is the byte offset of tile row r's first block; ntt = the number of 16-token
// MFMA tiles that hold a token; xrow(i), i < TT * 8 / 256, is the x row of tile token (tid + 256 i) >> 3 and yrow(tt),
// tt < TT / 16, the y row of tile token 16 tt + (lane & 15).  sb: TR * QL<QT>::SLOT bytes, sx: TT * KC * 2 bytes of LDS.
template <int QT, bool BF16, int TT, class XRow, class YRow>
__device__ __forceinline__ void tile_pass(const uint8_t* blocks, const int64_t* sbase, int nr, int ntt, int64_t r0, int64_t R,
                                          int64_t C, const uint8_t* x, XRow xrow, uint16_t* y, YRow yrow, uint8_t* sb,
                                          uint8_t* sx) {
    using Q = QL<QT>;
    using OutT = typename std::conditional<BF16, bf16_bits, half_bits>::type;
    constexpr int XP = TT * 8 / 256;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, q = lane >> 4;
    const int64_t nsb = C / 256;

    f32x4 acc[2][TT / 16];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int tt = 0; tt < TT / 16; ++tt) acc[a][tt] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x4 xr[XP];
    load_x<XP>(x, C, 0, xrow, xr);
    __syncthreads();  // sbase
    const uint8_t* B0 = sb + (32 * wave + l15) * Q::SLOT;
#pragma unroll 1
    for (int64_t j = 0; j < nsb; ++j) {
        stage_rows<QT>(blocks, sbase, j, nr, sb);  // (the barrier that ended the previous chunk freed sb)
#pragma unroll 1
        for (int c = 0; c < 256 / KC; ++c) {
#pragma unroll
            for (int i = 0; i < XP; ++i) {
                const int p = tid + 256 * i;
                *reinterpret_cast<u32x4*>(sx + ((p & 7) * TT + (p >> 3)) * 16) = xr[i];
            }
            __syncthreads();
            const int64_t kn = 256 * j + KC * (c + 1);
            if (kn < C) load_x<XP>(x, C, kn, xrow, xr);
            uint32_t w[2][8];
            decode16<QT, OutT>(B0, c, q, w[0]);
            decode16<QT, OutT>(B0 + 16 * Q::SLOT, c, q, w[1]);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const u32x4 wa = {w[0][4 * s], w[0][4 * s + 1], w[0][4 * s + 2], w[0][4 * s + 3]};
                const u32x4 wb = {w[1][4 * s], w[1][4 * s + 1], w[1][4 * s + 2], w[1][4 * s + 3]};
                const uint8_t* px = sx + ((2 * q + s) * TT + l15) * 16;
#pragma unroll
                for (int tt = 0; tt < TT / 16; ++tt)
                    if (tt < ntt) {
                        const u32x4 xa = *reinterpret_cast<const u32x4*>(px + tt * 256);
                        acc[0][tt] = mfma<BF16>(wa, xa, acc[0][tt]);
                        acc[1][tt] = mfma<BF16>(wb, xa, acc[1][tt]);
                    }
            }
            __syncthreads();  // sx (and after the last chunk sb) may be overwritten
        }
    }

    const bool vec = (R & 3) == 0;  // then (t R + r) * 2 is 8-byte aligned for r % 4 == 0
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int64_t r = r0 + 32 * wave + 16 * a + 4 * q;
#pragma unroll
        for (int tt = 0; tt < TT / 16; ++tt) {
            const Row t = yrow(tt);
            if (!t.on || r >= R) continue;
            uint16_t o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = cvt_out<OutT>(acc[a][tt][i]).b;
            uint16_t* py = y + t.row * R + r;
            if (vec) {
                *reinterpret_cast<uint2*>(py) = make_uint2((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16));
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (r + i < R) py[i] = o[i];
            }
        }
    }
}

}  // namespace gemmcore
}  // namespace gq
