// gq_codec.hip -- K7 (dequantize), K8 elementwise half (RTN quantize), K9-K13 (bit-packers).
//
// All HBM-bound byte/elementwise work: one pass over the inputs, 16-byte accesses.
//   dequantize : 1 B/param in (+ ~0.2 B of scales)  -> 2 or 4 B/param out
//   pack       : 1 B/param in                        -> type_size/256 B/param out
#include "gq_common.hpp"
#include "gq_pack_layout.hpp"

namespace gq {

// ------------------------------------------------------------------ dequantize
// reference quant_utils.py:277-310; one thread = 16 consecutive values (never
// straddles a group: G is 16 or 32).
template <typename OutT>
__device__ __forceinline__ OutT cvt_out(float v);
template <>
__device__ __forceinline__ float cvt_out<float>(float v) { return v; }
struct half_bits { uint16_t b; };
struct bf16_bits { uint16_t b; };
template <>
__device__ __forceinline__ half_bits cvt_out<half_bits>(float v) { return {f2h(v)}; }
template <>
__device__ __forceinline__ bf16_bits cvt_out<bf16_bits>(float v) { return {f2bf(v)}; }

template <typename OutT>
__global__ __launch_bounds__(256) void dequantize_kernel(
    const uint8_t* __restrict__ q, const uint16_t* __restrict__ d, const uint8_t* __restrict__ s,
    const uint16_t* __restrict__ dmin, const uint8_t* __restrict__ m, int64_t R, int64_t C, int G,
    int is_signed, OutT* __restrict__ out) {
    const int64_t n16 = R * C / 16;
    const int64_t per_row = C / 16;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / per_row, c = (i % per_row) * 16;
        const int64_t sg = r * (C / 256) + c / 256, g = r * (C / G) + c / G;
        const float ds = h2f(d[sg]) * ival(s[g], is_signed);
        const float dm = h2f(dmin[sg]) * ival(m[g], is_signed);
        const uint4 qv = *reinterpret_cast<const uint4*>(q + r * C + c);
        const uint32_t qw[4] = {qv.x, qv.y, qv.z, qv.w};
        OutT o[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            uint8_t b = (uint8_t)(qw[k >> 2] >> (8 * (k & 3)));
            o[k] = cvt_out<OutT>(dequantize1(ival(b, is_signed), ds, dm));
        }
        OutT* op = out + r * C + c;
        if constexpr (sizeof(OutT) == 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) reinterpret_cast<uint4*>(op)[k] = reinterpret_cast<const uint4*>(o)[k];
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) reinterpret_cast<uint4*>(op)[k] = reinterpret_cast<const uint4*>(o)[k];
        }
    }
}

int launch_dequantize(int q_type, const uint8_t* q, const uint16_t* d, const uint8_t* s, const uint16_t* dmin,
                      const uint8_t* m, int64_t R, int64_t C, void* out, int out_dtype, hipStream_t st) {
    TypeInfo ti;
    if (!type_info(q_type, ti)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_dequantize: unknown q_type %d", q_type);
    if (R <= 0 || C <= 0 || C % 256) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_dequantize: R=%ld C=%ld", (long)R, (long)C);
    const int64_t n16 = R * C / 16;
    dim3 grid((unsigned)((n16 + 255) / 256 < 8192 ? (n16 + 255) / 256 : 8192)), block(256);
    ProfScope ps(PT_DEQUANT, st);
    switch (out_dtype) {
    case GQ_F32:
        hipLaunchKernelGGL(dequantize_kernel<float>, grid, block, 0, st, q, d, s, dmin, m, R, C, ti.group,
                           ti.is_signed, (float*)out);
        break;
    case GQ_F16:
        hipLaunchKernelGGL(dequantize_kernel<half_bits>, grid, block, 0, st, q, d, s, dmin, m, R, C, ti.group,
                           ti.is_signed, (half_bits*)out);
        break;
    case GQ_BF16:
        hipLaunchKernelGGL(dequantize_kernel<bf16_bits>, grid, block, 0, st, q, d, s, dmin, m, R, C, ti.group,
                           ti.is_signed, (bf16_bits*)out);
        break;
    default: GQ_FAIL(GQ_E_BAD_TYPE, "gq_dequantize: unknown out_dtype %d", out_dtype);
    }
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

// ------------------------------------------------------------- RTN quantize
// reference quantizer.py:318-330: one vectorised quantize() over the unmodified
// weight with the per-group parameters expanded.  One thread = 16 values.
template <int WDT>
__device__ __forceinline__ float load_w(const void* W, int64_t idx) {
    if constexpr (WDT == GQ_F32) return reinterpret_cast<const float*>(W)[idx];
    else if constexpr (WDT == GQ_F16) return h2f(reinterpret_cast<const uint16_t*>(W)[idx]);
    else return bf2f(reinterpret_cast<const uint16_t*>(W)[idx]);
}

template <int WDT>
__global__ __launch_bounds__(256) void rtn_quantize_kernel(
    const void* __restrict__ W, const uint16_t* __restrict__ d, const uint8_t* __restrict__ s,
    const uint16_t* __restrict__ dmin, const uint8_t* __restrict__ m, int64_t R, int64_t C, int G, int is_signed,
    float qmin, float qmax, uint8_t* __restrict__ q) {
    const int64_t n16 = R * C / 16, per_row = C / 16;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / per_row, c = (i % per_row) * 16;
        const int64_t sg = r * (C / 256) + c / 256, g = r * (C / G) + c / G;
        const float ds = h2f(d[sg]) * ival(s[g], is_signed);
        const float dm = h2f(dmin[sg]) * ival(m[g], is_signed);
        uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            float v = quantize1(load_w<WDT>(W, r * C + c + k), ds, dm, qmin, qmax);
            uint8_t b = is_signed ? (uint8_t)(int8_t)v : (uint8_t)v;
            o[k >> 2] |= (uint32_t)b << (8 * (k & 3));
        }
        *reinterpret_cast<uint4*>(q + r * C + c) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

int launch_rtn_elementwise(const void* W, int w_dtype, const uint16_t* d, const uint8_t* s, const uint16_t* dmin,
                           const uint8_t* m, int64_t R, int64_t C, const TypeInfo& ti, uint8_t* q,
                           hipStream_t st) {
    const int64_t n16 = R * C / 16;
    dim3 grid((unsigned)((n16 + 255) / 256 < 8192 ? (n16 + 255) / 256 : 8192)), block(256);
    const float qmin = (float)ti.qmin, qmax = (float)ti.qmax;
    ProfScope ps(PT_RTN, st);
    switch (w_dtype) {
    case GQ_F32:
        hipLaunchKernelGGL(rtn_quantize_kernel<GQ_F32>, grid, block, 0, st, W, d, s, dmin, m, R, C, ti.group,
                           ti.is_signed, qmin, qmax, q);
        break;
    case GQ_F16:
        hipLaunchKernelGGL(rtn_quantize_kernel<GQ_F16>, grid, block, 0, st, W, d, s, dmin, m, R, C, ti.group,
                           ti.is_signed, qmin, qmax, q);
        break;
    case GQ_BF16:
        hipLaunchKernelGGL(rtn_quantize_kernel<GQ_BF16>, grid, block, 0, st, W, d, s, dmin, m, R, C, ti.group,
                           ti.is_signed, qmin, qmax, q);
        break;
    default: GQ_FAIL(GQ_E_BAD_TYPE, "gq_rtn_quantize: unknown w_dtype %d", w_dtype);
    }
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

// ---------------------------------------------------------------- bit-packers
// reference packing_utils.py:8-326.  A workgroup packs PB = 32 consecutive
// 256-value blocks per turn: the 32*256 input bytes are staged in LDS with coalesced
// 16-byte loads (two per thread in flight), every thread assembles FOUR consecutive
// output bytes from LDS and stores them as one dword, and the 32*type_size output
// bytes (a multiple of 16 for every type) leave as coalesced 16-byte stores.  (r01: 8
// blocks and byte-wide LDS stores per turn kept too few bytes in flight, 2.0-2.3 TB/s.)
// The layouts and the store of a turn live in gq_pack_layout.hpp (PB, pack_dword<QT>, pack_store<QT, TS, NG>).
template <int QT, int TS, int NG>
__global__ __launch_bounds__(256) void pack_kernel(const uint8_t* __restrict__ qw, const uint16_t* __restrict__ d,
                                                   const uint8_t* __restrict__ s, const uint16_t* __restrict__ dmin,
                                                   const uint8_t* __restrict__ m, int64_t nblocks,
                                                   uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t sq[PB * 256];
    __shared__ __attribute__((aligned(16))) uint8_t so[PB * TS];
    __shared__ __attribute__((aligned(16))) uint8_t ss[PB * NG];
    __shared__ __attribute__((aligned(16))) uint8_t sm[PB * NG];
    __shared__ uint16_t sd[PB], sdm[PB];
    const int tid = threadIdx.x;
    for (int64_t b0 = (int64_t)blockIdx.x * PB; b0 < nblocks; b0 += (int64_t)gridDim.x * PB) {
        const int nb = (int)((nblocks - b0) < PB ? (nblocks - b0) : PB);
        // stage inputs: nb*256 bytes = nb*16 uint4 (two loads per thread before the first LDS write)
        {
            const uint4* src = reinterpret_cast<const uint4*>(qw + b0 * 256);
            const int n16 = nb * 16;
            uint4 v0 = make_uint4(0, 0, 0, 0), v1 = v0;
            if (tid < n16) v0 = src[tid];
            if (tid + 256 < n16) v1 = src[tid + 256];
            if (tid < n16) reinterpret_cast<uint4*>(sq)[tid] = v0;
            if (tid + 256 < n16) reinterpret_cast<uint4*>(sq)[tid + 256] = v1;
        }
        for (int t = tid; t < nb * NG; t += 256) {
            ss[t] = s[b0 * NG + t];
            sm[t] = m ? m[b0 * NG + t] : 0;
        }
        if (tid < nb) {
            sd[tid] = d[b0 + tid];
            sdm[tid] = dmin ? dmin[b0 + tid] : 0;
        }
        __syncthreads();
        pack_store<QT, TS, NG>(sq, so, ss, sm, sd, sdm, nb, out + b0 * TS);
        __syncthreads();
    }
}

int launch_pack(int q_type, const uint8_t* q, const uint16_t* d, const uint8_t* s, const uint16_t* dmin,
                const uint8_t* m, int64_t R, int64_t C, uint8_t* out, hipStream_t st) {
    TypeInfo ti;
    if (!type_info(q_type, ti)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_pack: unknown q_type %d", q_type);
    if (R <= 0 || C <= 0 || C % 256) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_pack: R=%ld C=%ld (C %% 256 != 0)", (long)R, (long)C);
    if (!q || !d || !s || !out) GQ_FAIL(GQ_E_NULL, "gq_pack: null pointer");
    if (ti.k_search && (!dmin || !m)) GQ_FAIL(GQ_E_NULL, "gq_pack: dmin/m required for q_type %d", q_type);
    const int64_t nblocks = R * (C / 256);
    int64_t g = (nblocks + PB - 1) / PB;
    dim3 grid((unsigned)(g < 4096 ? g : 4096)), block(256);  // (1024 .. 16384 workgroups measured: no difference from 2048 up)
    ProfScope ps(PT_PACK, st);
    switch (q_type) {
    case GQ_Q2_K: hipLaunchKernelGGL((pack_kernel<GQ_Q2_K, 84, 16>), grid, block, 0, st, q, d, s, dmin, m, nblocks, out); break;
    case GQ_Q3_K: hipLaunchKernelGGL((pack_kernel<GQ_Q3_K, 110, 16>), grid, block, 0, st, q, d, s, dmin, m, nblocks, out); break;
    case GQ_Q4_K: hipLaunchKernelGGL((pack_kernel<GQ_Q4_K, 144, 8>), grid, block, 0, st, q, d, s, dmin, m, nblocks, out); break;
    case GQ_Q5_K: hipLaunchKernelGGL((pack_kernel<GQ_Q5_K, 176, 8>), grid, block, 0, st, q, d, s, dmin, m, nblocks, out); break;
    case GQ_Q6_K: hipLaunchKernelGGL((pack_kernel<GQ_Q6_K, 210, 16>), grid, block, 0, st, q, d, s, dmin, m, nblocks, out); break;
    }
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // namespace gq
