// gq_iq4_search.hpp -- the scale search of include/gptq_gguf_iq4_encode.h as device functions: ONE text for the encoder
// (gq_iq4_encode.hip, one lane per 32-value block), the lazy scale step of the column walk on the IQ4 grid (gq_iq4_gptq.hip,
// one lane per CANDIDATE) and the segment kernel's per-column rounding (gq_gptq.hip).  Every function is one operation of the
// header's contract (fp32, each operation rounded on its own, sums in ascending j).
#pragma once

#include "../gq_common.hpp"

namespace gq {
namespace iq4 {

// kv and a sentinel above every finite product: best() reads kvs[u + 1] with u up to 15
__device__ const float KV17[17] = {-127.f, -104.f, -83.f, -65.f, -49.f, -35.f, -22.f, -10.f, 1.f,
                                   13.f,   25.f,   38.f,  53.f,  69.f,  89.f,  113.f, 3.0e38f};

// best(a) of the header -> (index, kv[index]).  u counts the entries <= a by binary search, so kv[u] <= a < kv[u + 1] inside the
// table; below it u = 0 and (a - kv[0]) < 0 picks 0, above it u = 15 and the sentinel picks 15.  The two rounded differences are
// compared, a tie goes up.  kvs: KV17 in LDS.
__device__ __forceinline__ void best(const float* __restrict__ kvs, float a, int& idx, float& q) {
    int u = a >= 1.0f ? 8 : 0;  // kv[8]
    u += a >= kvs[u + 4] ? 4 : 0;
    u += a >= kvs[u + 2] ? 2 : 0;
    u += a >= kvs[u + 1] ? 1 : 0;
    const float lo = kvs[u], hi = kvs[u + 1];
    const bool down = (a - lo) < (hi - a);
    idx = down ? u : u + 1;
    q = down ? lo : hi;
}

// The same best(a) without a table in LDS or memory, for a dependent chain (wave 0 of the column walk): u is the COUNT of the
// fifteen compares a >= kv[i] -- independent of one another, each consumed at once by an add-with-carry -- and kv[u], kv[u + 1]
// come out of register-resident byte tables (kv + 128 fits a byte) by v_perm_b32, as the decode side does it.  Then the two
// rounded differences as above.  At u == 15 the upper table repeats kv[15]: (a - 113) < (113 - a) is false for every
// a >= 113, so the "up" side is taken with the index clamped to 15 -- kv[15] either way, as the sentinel gives it.
// The constants are held in VGPRs on purpose (init() makes them opaque): as literals the compiler keeps them in SGPRs across
// the unrolled chain, and the segment kernel has none to spare (sgpr_spill_count 489 that way, 0 this way).
struct BestReg {
    float k[15];
    uint32_t lo4[4], hi4[4];
    static constexpr int KV[17] = {-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113, 113};
    static constexpr uint32_t word(int i0) {
        return (uint32_t)(KV[i0] + 128) | (uint32_t)(KV[i0 + 1] + 128) << 8 | (uint32_t)(KV[i0 + 2] + 128) << 16 |
               (uint32_t)(KV[i0 + 3] + 128) << 24;
    }
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int i = 0; i < 15; ++i) {
            k[i] = (float)KV[i + 1];
            asm volatile("" : "+v"(k[i]));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lo4[i] = word(4 * i), hi4[i] = word(4 * i + 1);
            asm volatile("" : "+v"(lo4[i]), "+v"(hi4[i]));
        }
    }
    __device__ __forceinline__ void best(float a, int& idx, float& q) const {
        int u = 0;
#pragma unroll
        for (int i = 0; i < 15; ++i) u += a >= k[i] ? 1 : 0;
        const bool upper = u >= 8;
        const uint32_t sel = (uint32_t)u & 7u;
        const uint32_t lob = __builtin_amdgcn_perm(upper ? lo4[3] : lo4[1], upper ? lo4[2] : lo4[0], sel);
        const uint32_t hib = __builtin_amdgcn_perm(upper ? hi4[3] : hi4[1], upper ? hi4[2] : hi4[0], sel);
        const float lo = (float)(lob & 0xffu) - 128.0f, hi = (float)(hib & 0xffu) - 128.0f;
        const bool down = (a - lo) < (hi - a);
        const int up = u + 1 < 15 ? u + 1 : 15;
        idx = down ? u : up;
        q = down ? lo : hi;
    }
};

// sigma2 of a super-block of `size` values from the sum s of their squares
__device__ __forceinline__ float sigma2_of(float s, float size) { return s * (2.0f / size); }

// the weights of a block: importance * sqrtf(sigma2 + x^2), or x^2 without importance / with all of it zero over the block
__device__ __forceinline__ float weight_of(float x, float imp, float sigma2, bool weighted) {
    return weighted ? imp * sqrtf(sigma2 + x * x) : x * x;
}

// amax and the signed value at the FIRST j that reaches it
__device__ __forceinline__ void block_max(const float (&xv)[32], float& amax, float& mx) {
    amax = 0.0f, mx = 0.0f;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const float ax = fabsf(xv[j]);
        if (ax > amax) amax = ax, mx = xv[j];
    }
}

// the inverse scale of candidate itry = -8 .. 7 (-8: the first candidate 1 / d0, always taken)
__device__ __forceinline__ float cand_id(int itry, float mx) {
    const float d0 = -mx / -127.0f;
    return itry == -8 ? 1.0f / d0 : ((float)itry + -127.0f) / mx;
}

__device__ __forceinline__ void cand_sums(const float* __restrict__ kvs, const float (&xv)[32], const float (&w)[32], float id,
                                          float& sumqx, float& sumq2) {
    sumqx = 0.0f, sumq2 = 0.0f;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        int idx;
        float q;
        best(kvs, id * xv[j], idx, q);
        const float wq = w[j] * q;
        sumqx += wq * xv[j];
        sumq2 += wq * q;
    }
}

// the selection, in the order itry = -8, -7, .., 7
__device__ __forceinline__ void cand_take(int itry, float sumqx, float sumq2, float& d, float& bst) {
    if (itry == -8 || (sumq2 > 0.0f && sumqx * sumqx > bst * sumq2)) {
        d = sumqx / sumq2;
        bst = d * sumqx;
    }
}

// IQ4_XS: D from ms (the block scale of largest |d|, the first one on a tie); then l, dl and idl of a block with scale d
__device__ __forceinline__ float xs_super_scale(float ms) { return -ms / 32.0f; }
__device__ __forceinline__ void xs_block_scale(float D, float d, float& lf, float& dl, float& idl) {
    const float iD = D != 0.0f ? 1.0f / D : 0.0f;
    lf = fminf(fmaxf(rintf(iD * d), -32.0f), 31.0f);
    dl = D * lf;
    idl = dl != 0.0f ? 1.0f / dl : 0.0f;
}
__device__ __forceinline__ float nl_inverse(float d) { return d != 0.0f ? 1.0f / d : 0.0f; }

}  // namespace iq4
}  // namespace gq
