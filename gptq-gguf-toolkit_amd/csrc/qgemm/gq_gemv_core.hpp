// gq_gemv_core.hpp -- the one text of the packed GEMV: K loop, wave-order reduction and store of a workgroup that owns 16 rows
// of a packed weight and all of C.  gq_qgemv.hip (K22, MFMA column t = token t) and gq_moe_gemv.hip (K24, MFMA column i = the
// i-th pair that names the workgroup's expert) include it, so for one weight row and one input row the two kernels run the
// same instructions in the same order: the same bits.  The form is described at the head of gq_qgemv.hip.
// Device code only: the entry points' type dispatch and operand checks are search/gq_block_host.hpp's.
#pragma once
#include <type_traits>

#include "../search/gq_block_decode.hpp"

namespace gq {
namespace gemvcore {

using namespace blockdec;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int VR = 16;      // rows of a workgroup (one MFMA tile)
constexpr int MAX_NW = 16;  // waves of a workgroup: the K split

template <int QT> constexpr int smem_bytes() { return MAX_NW * VR * QL<QT>::SLOT; }  // a wave's VR slots at wave * VR * SLOT

template <bool BF16>
__device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
    if constexpr (BF16)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// the LDS accesses of one wave to its own slots, in program order for every lane of it
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Stage superblock j of the workgroup's nr rows into the wave's slots sb: lane r (< 16) holds in `base` the byte offset of row
// r's first block, the other lanes fetch it by shuffle.
template <int QT>
__device__ __forceinline__ void stage_wave(const uint8_t* __restrict__ blocks, int64_t base, int64_t j, int nr, int lane,
                                           uint8_t* sb) {
    using Q = QL<QT>;
    using U = typename std::conditional<Q::AL == 16, u32x4, typename Unit<Q::AL>::T>::type;  // (a vector type stays in registers)
    // 3 (Q4_K) .. 34 (Q8_0) loads per lane, in groups of at most 17 that are all in flight before the group's first LDS write
    // (all 27 or 34 at once spill; measured, groups of 8 are no slower: the 2-byte types pay for the number of loads)
    constexpr int NIT = (VR * Q::UPR + 63) / 64, GRP = NIT < 17 ? NIT : 17;
    const int n = nr * Q::UPR;
#pragma unroll 1
    for (int it0 = 0; it0 < NIT; it0 += GRP) {
        U v[GRP] = {};
#pragma unroll
        for (int g = 0; g < GRP; ++g) {
            const int u = lane + 64 * (it0 + g), r = u / Q::UPR, o = u - r * Q::UPR;
            const int64_t rb = __shfl(base, r & (VR - 1));  // (every lane takes part; r < 16 where u < n)
            if (it0 + g < NIT && u < n) v[g] = *reinterpret_cast<const U*>(blocks + rb + j * Q::ROWB + o * Q::AL);
        }
#pragma unroll
        for (int g = 0; g < GRP; ++g) {
            const int u = lane + 64 * (it0 + g), r = u / Q::UPR, o = u - r * Q::UPR;
            if (it0 + g < NIT && u < n) *reinterpret_cast<U*>(sb + r * Q::SLOT + Q::lds_off(o)) = v[g];
        }
    }
}

// One pass of a workgroup of blockDim.x / 64 waves (tid: the caller's threadIdx.x): D[r][i] = sum_c W[r0 + r][c] * X_i[c] for its nr rows (row l15's first
// block at blocks + base, held by the lanes l15 < nr) and up to 16 input rows, one per MFMA column.  Lane (l15, q) serves
// column i = l15: `on` says whether the column carries an input row, xi is that row of x (rows of C elements) and yi() the row
// of y (rows of R elements; asked for after the reduction, so that it need not live through the K loop) whose elements r0 .. r0 + nr - 1 the column writes; both are used only where `on`.  smem: smem_bytes<QT>()
// bytes, 16-byte aligned.  The only workgroup barrier sits between the K loop and the reduction; a caller that makes another
// pass puts one between the passes (wave 0 reads every wave's slots until it returns from here).
template <int QT, bool BF16, class YRow>
__device__ __forceinline__ void gemv_pass(int tid, const uint8_t* __restrict__ blocks, int64_t base, int nr, int64_t r0, int64_t R,
                                          int64_t C, bool on, const uint8_t* __restrict__ x, int xi, uint16_t* __restrict__ y, YRow yi,
                                          uint8_t* smem) {
    using Q = QL<QT>;
    using OutT = typename std::conditional<BF16, bf16_bits, half_bits>::type;
    static_assert(VR * Q::SLOT >= 64 * 16, "a wave's slots hold its partial sums");
    const int lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6, l15 = lane & 15, q = lane >> 4;
    uint8_t* sb = smem + wave * VR * Q::SLOT;
    const int64_t nsb = C / 256;

    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const uint8_t* B = sb + l15 * Q::SLOT;
    const uint8_t* xl = x + ((int64_t)xi * C + 16 * q) * 2;
#pragma unroll 1
    for (int64_t j = wave; j < nsb; j += nw) {
        u32x4 xr[2], xn[2] = {};  // piece s of chunk c: x[256 j + 64 c + 16 q + 8 s .. + 7]
#pragma unroll
        for (int s = 0; s < 2; ++s) xr[s] = on ? *reinterpret_cast<const u32x4*>(xl + (256 * j + 8 * s) * 2) : u32x4{0, 0, 0, 0};
        stage_wave<QT>(blocks, base, j, nr, lane, sb);
        wave_sync();
#pragma unroll 1
        for (int c = 0; c < 4; ++c) {
            if (c < 3 && on) {  // the next chunk's x is in flight during this chunk's decode
#pragma unroll
                for (int s = 0; s < 2; ++s) xn[s] = *reinterpret_cast<const u32x4*>(xl + (256 * j + 64 * (c + 1) + 8 * s) * 2);
            }
            uint32_t w[8];
            decode16<QT, OutT>(B, c, q, w);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                acc = mfma<BF16>(u32x4{w[4 * s], w[4 * s + 1], w[4 * s + 2], w[4 * s + 3]}, xr[s], acc);
                xr[s] = xn[s];
            }
        }
        wave_sync();  // the slots may be overwritten
    }

    *reinterpret_cast<f32x4*>(sb + lane * 16) = acc;
    __syncthreads();
    if (wave != 0) return;
    acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int w = 0; w < nw; ++w) {  // wave order: the same bits every call
        const f32x4 p = *reinterpret_cast<const f32x4*>(smem + w * VR * Q::SLOT + lane * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += p[i];
    }
    const int64_t r = r0 + 4 * q;
    if (!on || r >= R) return;
    uint16_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = cvt_out<OutT>(acc[i]).b;
    uint16_t* py = y + (int64_t)yi() * R + r;
    if ((R & 3) == 0) {  // then (row * R + r) * 2 is 8-byte aligned for r % 4 == 0
        *reinterpret_cast<uint2*>(py) = make_uint2((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16));
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (r + i < R) py[i] = o[i];
    }
}

}  // namespace gemvcore
}  // namespace gq
