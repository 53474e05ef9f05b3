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
//
// Q8_0 (include/gptq_gguf_q8.h; dequantize_row_q8_0) takes the same route through gq_dequantize_blocks: a turn is 128 blocks of
// 32 values, staged by 2-byte loads into 48-byte LDS slots, half a block per thread, w = f32(d) * f32(q) and one cast
// (blockdec::decode_turn_b32).  gq_unpack has no Q8_0 form: the five data.pth tensors are a K-quant notion.
//
// IQ4_NL and IQ4_XS (include/gptq_gguf_iq4.h; dequantize_row_iq4_nl / _iq4_xs): w = f32(d) * f32(ls - 32) * f32(kv[code]), both
// products exact, one cast.  IQ4_XS is a 256-value type and takes the K-quants' route (decode_turn): 8-byte staging loads -- 136
// = 17 x 8 -- into a 144-byte slot with the block at byte 8, so that the 16 code bytes of a thread are one aligned 16-byte LDS
// read; ds = d * (ls - 32), dm = 0 and the code is kv[nibble], looked up in a register-resident table with byte permutes
// (blockdec::iq4_code4).  IQ4_NL is a 32-value type and takes Q8_0's route: 2-byte staging loads, half a block per thread.
// Neither has a gq_unpack form.
#include "../search/gq_block_host.hpp"  // gq_block_decode.hpp (Lay, stage_blocks, codes16, group_scale, decode_turn: shared with
                                        // search/gq_switch.hip) and the host side: the type list and its geometry

namespace gq {
namespace {

using namespace blockdec;

// four independent byte additions (no carry across bytes)
__device__ __forceinline__ uint32_t add4(uint32_t x, uint32_t c) {
    return ((x & 0x7f7f7f7fu) + (c & 0x7f7f7f7fu)) ^ ((x ^ c) & 0x80808080u);
}

template <int QT, typename OutT>
__global__ __launch_bounds__(256) void dequantize_blocks_kernel(const uint8_t* __restrict__ blocks,
                                                                const int32_t* __restrict__ row_src, int64_t nblocks,
                                                                int64_t nbr, OutT* __restrict__ out) {
    using L = Lay<QT>;
    __shared__ __attribute__((aligned(16))) uint8_t sb[DB * L::TSP];
    __shared__ int64_t ssrc[DB];
    for (int64_t b0 = (int64_t)blockIdx.x * DB; b0 < nblocks; b0 += (int64_t)gridDim.x * DB) {
        const int nb = (int)((nblocks - b0) < DB ? (nblocks - b0) : DB);
        decode_turn<QT, OutT>(blocks, row_src, b0, nb, nbr, out, sb, ssrc);
        __syncthreads();
    }
}

// Q8_0 (include/gptq_gguf_q8.h), IQ4_NL (include/gptq_gguf_iq4.h): the same loop over turns of 128 blocks of 32 values,
// w = f32(d) * f32(q) and one cast
template <int QT, typename OutT>
__global__ __launch_bounds__(256) void dequantize_b32_kernel(const uint8_t* __restrict__ blocks,
                                                             const int32_t* __restrict__ row_src, int64_t nblocks,
                                                             int64_t nbr, OutT* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t sb[B32_DB * B32_SLOT];
    __shared__ int64_t ssrc[B32_DB];
    for (int64_t b0 = (int64_t)blockIdx.x * B32_DB; b0 < nblocks; b0 += (int64_t)gridDim.x * B32_DB) {
        const int nb = (int)((nblocks - b0) < B32_DB ? (nblocks - b0) : B32_DB);
        decode_turn_b32<QT, OutT>(blocks, row_src, b0, nb, nbr, out, sb, ssrc);
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

unsigned turns_grid(int64_t nblocks, int per_turn = DB) {
    const int64_t g = (nblocks + per_turn - 1) / per_turn;
    return (unsigned)(g < 16384 ? g : 16384);
}

template <int QT>
int launch_dequantize(const uint8_t* blocks, const int32_t* row_src, int64_t nblocks, int64_t nbr, void* out, int out_dtype,
                      hipStream_t st) {
    constexpr bool B32 = Geo<QT>::BS == 32;  // Q8_0, IQ4_NL: turns of 128 blocks of 32 values
    if (!aligned(blocks, QL<QT>::AL)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_dequantize_blocks: blocks not %d-byte aligned", QL<QT>::AL);
    const dim3 grid(turns_grid(nblocks, B32 ? B32_DB : DB)), block(256);
    auto go = [&](auto* o) {
        using OutT = std::remove_pointer_t<decltype(o)>;
        if constexpr (B32) hipLaunchKernelGGL((dequantize_b32_kernel<QT, OutT>), grid, block, 0, st, blocks, row_src, nblocks, nbr, o);
        else hipLaunchKernelGGL((dequantize_blocks_kernel<QT, OutT>), grid, block, 0, st, blocks, row_src, nblocks, nbr, o);
    };
    switch (out_dtype) {
    case GQ_F32: go((float*)out); break;
    case GQ_F16: go((half_bits*)out); break;
    default: go((bf16_bits*)out); break;
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
    if (!packed_type(q_type)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_dequantize_blocks: unknown q_type %d", q_type);
    const int bs = block_geometry(q_type).bs;  // values per block
    if (out_dtype != GQ_F32 && out_dtype != GQ_F16 && out_dtype != GQ_BF16)
        GQ_FAIL(GQ_E_BAD_TYPE, "gq_dequantize_blocks: unknown out_dtype %d", out_dtype);
    if (R <= 0 || C <= 0 || C % bs)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_dequantize_blocks: R=%ld C=%ld (C %% %d != 0)", (long)R, (long)C, bs);
    if (!blocks || !out) GQ_FAIL(GQ_E_NULL, "gq_dequantize_blocks: null pointer");
    if (!aligned(out, 16)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_dequantize_blocks: out must be 16-byte aligned");
    const int64_t nbr = C / bs, nblocks = R * nbr;
    hipStream_t st = (hipStream_t)stream;
    int rc = GQ_OK;
    dispatch_packed(q_type, [&](auto qt) { rc = launch_dequantize<decltype(qt)::value>(blocks, row_src, nblocks, nbr, out, out_dtype, st); });
    return rc;
}

}  // extern "C"
