// gq_decode.hip -- K15: the inverse of the bit-packers (K9-K13).  block_q{2..6}_K bytes -> the five data.pth tensors
// (gq_unpack), or straight to weights (gq_dequantize_blocks: decode + quant_utils.py:277-310 + cast in one pass).
//
// HBM-bound streaming, the writes dominate:
//   dequantize_blocks : type_size/256 B/param in (0.33-0.82) -> 2 or 4 B/param out
//   unpack            : the same in                          -> 1 B/param + ~0.1-0.2 B of scales out
// pack_kernel in reverse.  A workgroup takes DB = 16 consecutive blocks of the OUTPUT per turn (output block L = r * C/256
// + j; its bytes are block j of packed row row_src[r]) and stages them in LDS, every block at a 16-byte aligned slot of
// TSP = round-up(type_size, 16) bytes.  A block of the 110- / 210-byte layouts (and a gathered row of them) is only 2-byte
// aligned in global memory and an 84-byte one 4-byte aligned: the staging loads are AL = 2 / 4 / 16 bytes wide, the natural
// alignment of the type, and cover exactly the block's bytes -- nothing outside [blocks, blocks + R * rowbytes) is read.
// Then thread (b, g) = (tid / 16, tid % 16) produces the 16 consecutive values 16 g .. 16 g + 15 of block b (one scale
// group, or half of one) from two 16-byte LDS reads with byte-parallel shifts and masks, and stores them as 1 (bytes),
// 2 (fp16 / bf16) or 4 (fp32) 16-byte stores; consecutive lanes write consecutive 16 / 32 / 64 bytes.
//
// Numerical contract (exact class): ds = f32(d) * f32(sc), dm = f32(dmin) * f32(mn), w = ds * f32(code) - dm, every
// operation rounded on its own (-ffp-contract=off), then one round-to-nearest-even cast: dequantize1 of gq_common.hpp on
// the decoded fields.  Q3_K / Q6_K have no minimum: dm = 0 * 0 = +0 and x - (+0) == x for every x, -0 included.
// Layouts: llama.cpp ggml-quants.c dequantize_row_q{2,3,4,5,6}_K and get_scale_min_k4.
#include "../gq_common.hpp"

namespace gq {
namespace {

constexpr int DB = 16;  // blocks per turn: 256 threads x 16 values

template <int QT> struct Lay;
//                                  type_size, LDS slot, staging width, scale groups, offset of the stored code
template <> struct Lay<GQ_Q2_K> { static constexpr int TS = 84, TSP = 96, AL = 4, NG = 16, OFF = 0; };
template <> struct Lay<GQ_Q3_K> { static constexpr int TS = 110, TSP = 112, AL = 2, NG = 16, OFF = 4; };
template <> struct Lay<GQ_Q4_K> { static constexpr int TS = 144, TSP = 144, AL = 16, NG = 8, OFF = 0; };
template <> struct Lay<GQ_Q5_K> { static constexpr int TS = 176, TSP = 176, AL = 16, NG = 8, OFF = 0; };
template <> struct Lay<GQ_Q6_K> { static constexpr int TS = 210, TSP = 224, AL = 2, NG = 16, OFF = 32; };

template <int AL> struct Unit;
template <> struct Unit<2> { using T = uint16_t; };
template <> struct Unit<4> { using T = uint32_t; };
template <> struct Unit<16> { using T = uint4; };

__device__ __forceinline__ uint32_t ld4(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }
__device__ __forceinline__ uint16_t ld2(const uint8_t* p) { return *reinterpret_cast<const uint16_t*>(p); }
__device__ __forceinline__ void ld16(const uint8_t* p, uint32_t w[4]) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
}
// four independent byte additions (no carry across bytes)
__device__ __forceinline__ uint32_t add4(uint32_t x, uint32_t c) {
    return ((x & 0x7f7f7f7fu) + (c & 0x7f7f7f7fu)) ^ ((x ^ c) & 0x80808080u);
}

// (d, dmin) bits of the block at LDS slot B
template <int QT>
__device__ __forceinline__ void block_d(const uint8_t* B, uint16_t& d, uint16_t& dmin) {
    if constexpr (QT == GQ_Q2_K) d = ld2(B + 80), dmin = ld2(B + 82);
    else if constexpr (QT == GQ_Q3_K) d = ld2(B + 108), dmin = 0;
    else if constexpr (QT == GQ_Q6_K) d = ld2(B + 208), dmin = 0;
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

// the 16 codes 16 g16 .. 16 g16 + 15 of the block, one per byte, as stored (Q3_K: code + 4, Q6_K: code + 32)
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
        if (u < nb * UPB) *reinterpret_cast<U*>(sb + b * L::TSP + o * L::AL) = v[it];
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

template <int QT, typename OutT>
__global__ __launch_bounds__(256) void dequantize_blocks_kernel(const uint8_t* __restrict__ blocks,
                                                                const int32_t* __restrict__ row_src, int64_t nblocks,
                                                                int64_t nbr, OutT* __restrict__ out) {
    using L = Lay<QT>;
    __shared__ __attribute__((aligned(16))) uint8_t sb[DB * L::TSP];
    __shared__ int64_t ssrc[DB];
    const int tid = threadIdx.x, b = tid >> 4, g16 = tid & 15;
    for (int64_t b0 = (int64_t)blockIdx.x * DB; b0 < nblocks; b0 += (int64_t)gridDim.x * DB) {
        const int nb = (int)((nblocks - b0) < DB ? (nblocks - b0) : DB);
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
        __syncthreads();
    }
}

template <int QT>
__global__ __launch_bounds__(256) void unpack_kernel(const uint8_t* __restrict__ blocks, int64_t nblocks,
                                                     uint8_t* __restrict__ qw, uint16_t* __restrict__ d,
                                                     uint8_t* __restrict__ s, uint16_t* __restrict__ dmin,
                                                     uint8_t* __restrict__ m) {
    using L = Lay<QT>;
    __shared__ __attribute__((aligned(16))) uint8_t sb[DB * L::TSP];
    __shared__ int64_t ssrc[DB];
    const int tid = threadIdx.x, b = tid >> 4, g16 = tid & 15;
    for (int64_t b0 = (int64_t)blockIdx.x * DB; b0 < nblocks; b0 += (int64_t)gridDim.x * DB) {
        const int nb = (int)((nblocks - b0) < DB ? (nblocks - b0) : DB);
        stage_blocks<QT>(blocks, nullptr, b0, nb, nblocks, sb, ssrc);
        if (b < nb) {
            uint32_t c[4];
            codes16<QT>(sb + b * L::TSP, g16, c);
            if constexpr (L::OFF != 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) c[i] = add4(c[i], 0x01010101u * (uint32_t)(256 - L::OFF));  // int8 in the byte
            }
            *reinterpret_cast<uint4*>(qw + (b0 + b) * 256 + 16 * g16) = make_uint4(c[0], c[1], c[2], c[3]);
        }
        // the scale / min bytes, four groups per thread (one dword store each); d / dmin, one block per thread
        constexpr int WPB = L::NG / 4;
        if (tid < nb * WPB) {
            const int bb = tid / WPB, w = tid - bb * WPB;
            uint32_t sv = 0, mv = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int sc, mn;
                group_scale<QT>(sb + bb * L::TSP, 4 * w + k, sc, mn);
                sv |= (uint32_t)(uint8_t)sc << (8 * k);
                mv |= (uint32_t)(uint8_t)mn << (8 * k);
            }
            reinterpret_cast<uint32_t*>(s)[b0 * WPB + tid] = sv;
            if (m) reinterpret_cast<uint32_t*>(m)[b0 * WPB + tid] = mv;
        }
        if (tid >= 128 && tid - 128 < nb) {
            uint16_t dv, dmv;
            block_d<QT>(sb + (tid - 128) * L::TSP, dv, dmv);
            d[b0 + tid - 128] = dv;
            if (dmin) dmin[b0 + tid - 128] = dmv;
        }
        __syncthreads();
    }
}

unsigned turns_grid(int64_t nblocks) {
    const int64_t g = (nblocks + DB - 1) / DB;
    return (unsigned)(g < 16384 ? g : 16384);
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <int QT>
int launch_dequantize_blocks_t(const uint8_t* blocks, const int32_t* row_src, int64_t nblocks, int64_t nbr, void* out,
                               int out_dtype, hipStream_t st) {
    if (!aligned(blocks, Lay<QT>::AL)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_dequantize_blocks: blocks not %d-byte aligned", Lay<QT>::AL);
    dim3 grid(turns_grid(nblocks)), block(256);
    switch (out_dtype) {
    case GQ_F32:
        hipLaunchKernelGGL((dequantize_blocks_kernel<QT, float>), grid, block, 0, st, blocks, row_src, nblocks, nbr, (float*)out);
        break;
    case GQ_F16:
        hipLaunchKernelGGL((dequantize_blocks_kernel<QT, half_bits>), grid, block, 0, st, blocks, row_src, nblocks, nbr,
                           (half_bits*)out);
        break;
    default:
        hipLaunchKernelGGL((dequantize_blocks_kernel<QT, bf16_bits>), grid, block, 0, st, blocks, row_src, nblocks, nbr,
                           (bf16_bits*)out);
        break;
    }
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

template <int QT>
int launch_unpack_t(const uint8_t* blocks, int64_t nblocks, uint8_t* qw, uint16_t* d, uint8_t* s, uint16_t* dmin, uint8_t* m,
                    hipStream_t st) {
    if (!aligned(blocks, Lay<QT>::AL)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_unpack: blocks not %d-byte aligned", Lay<QT>::AL);
    hipLaunchKernelGGL((unpack_kernel<QT>), dim3(turns_grid(nblocks)), dim3(256), 0, st, blocks, nblocks, qw, d, s, dmin, m);
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_unpack(int q_type, const uint8_t* blocks, int64_t R, int64_t C, uint8_t* qweight, uint16_t* d, uint8_t* s,
              uint16_t* dmin, uint8_t* m, void* stream) {
    if (int rc = options_ok()) return rc;
    TypeInfo ti;
    if (!type_info(q_type, ti)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_unpack: unknown q_type %d", q_type);
    if (R <= 0 || C <= 0 || C % 256) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_unpack: R=%ld C=%ld (C %% 256 != 0)", (long)R, (long)C);
    if (!blocks || !qweight || !d || !s) GQ_FAIL(GQ_E_NULL, "gq_unpack: null pointer");
    if (ti.k_search && (!dmin || !m)) GQ_FAIL(GQ_E_NULL, "gq_unpack: dmin/m required for q_type %d", q_type);
    if (!aligned(qweight, 16) || !aligned(s, 4) || !aligned(m, 4) || !aligned(d, 2) || !aligned(dmin, 2))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_unpack: outputs must be aligned (qweight 16 bytes, s / m 4, d / dmin 2)");
    const int64_t nblocks = R * (C / 256);
    hipStream_t st = (hipStream_t)stream;
    switch (q_type) {
    case GQ_Q2_K: return launch_unpack_t<GQ_Q2_K>(blocks, nblocks, qweight, d, s, dmin, m, st);
    case GQ_Q3_K: return launch_unpack_t<GQ_Q3_K>(blocks, nblocks, qweight, d, s, dmin, m, st);
    case GQ_Q4_K: return launch_unpack_t<GQ_Q4_K>(blocks, nblocks, qweight, d, s, dmin, m, st);
    case GQ_Q5_K: return launch_unpack_t<GQ_Q5_K>(blocks, nblocks, qweight, d, s, dmin, m, st);
    default: return launch_unpack_t<GQ_Q6_K>(blocks, nblocks, qweight, d, s, dmin, m, st);
    }
}

int gq_dequantize_blocks(int q_type, const uint8_t* blocks, int64_t R, int64_t C, const int32_t* row_src, void* out,
                         int out_dtype, void* stream) {
    if (int rc = options_ok()) return rc;
    TypeInfo ti;
    if (!type_info(q_type, ti)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_dequantize_blocks: unknown q_type %d", q_type);
    if (out_dtype != GQ_F32 && out_dtype != GQ_F16 && out_dtype != GQ_BF16)
        GQ_FAIL(GQ_E_BAD_TYPE, "gq_dequantize_blocks: unknown out_dtype %d", out_dtype);
    if (R <= 0 || C <= 0 || C % 256)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_dequantize_blocks: R=%ld C=%ld (C %% 256 != 0)", (long)R, (long)C);
    if (!blocks || !out) GQ_FAIL(GQ_E_NULL, "gq_dequantize_blocks: null pointer");
    if (!aligned(out, 16)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_dequantize_blocks: out must be 16-byte aligned");
    const int64_t nbr = C / 256, nblocks = R * nbr;
    hipStream_t st = (hipStream_t)stream;
    switch (q_type) {
    case GQ_Q2_K: return launch_dequantize_blocks_t<GQ_Q2_K>(blocks, row_src, nblocks, nbr, out, out_dtype, st);
    case GQ_Q3_K: return launch_dequantize_blocks_t<GQ_Q3_K>(blocks, row_src, nblocks, nbr, out, out_dtype, st);
    case GQ_Q4_K: return launch_dequantize_blocks_t<GQ_Q4_K>(blocks, row_src, nblocks, nbr, out, out_dtype, st);
    case GQ_Q5_K: return launch_dequantize_blocks_t<GQ_Q5_K>(blocks, row_src, nblocks, nbr, out, out_dtype, st);
    default: return launch_dequantize_blocks_t<GQ_Q6_K>(blocks, row_src, nblocks, nbr, out, out_dtype, st);
    }
}

}  // extern "C"
