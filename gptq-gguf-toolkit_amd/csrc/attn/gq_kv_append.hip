// gq_kv_append.hip -- K33: the append of a Q8_0 KV cache (include/gptq_gguf_kvcache.h).  The T new K rows and the T new V rows
// of every (b, h) are encoded into positions pos0 .. pos0 + T - 1 of the two caches in ONE launch (blockIdx.y = 0: K, 1: V),
// read through the strides of the attention layer's transposed view -- no .contiguous() copy.
//
// The arithmetic is K20's (q8/gq_q8_0.hip), so the bytes are gq_quantize_q8_0's: thread (block, h) = (id / 2, id % 2) reads the
// 16 consecutive values of half h of one 32-value block with two 16-byte loads (rows start 16-byte aligned: the base is, and
// every stride is a multiple of 8 elements), widens them exactly, takes the block's amax as the max over its registers and
// one exchange with lane id ^ 1, and both lanes compute the same d, id and their 16 codes.  A decode step writes B Hkv D / 32
// blocks of 34 bytes scattered over the (b, h) slabs, 2-byte aligned: the codes go out as 2-byte stores that cover exactly the
// rows, with no LDS image -- at T = 1 a slab receives 68 or 136 bytes, there is no span to gather.  (A prefill of thousands of
// rows pays for the narrow stores; it runs once per sequence.)
//
// Numerical contract (exact class; -ffp-contract=off): gptq_gguf_q8.h's.
#include "../../../include/gptq_gguf_kvcache.h"

#include "../search/gq_block_host.hpp"

namespace gq {
namespace {

template <bool BF16>
__global__ __launch_bounds__(256) void kv_append_kernel(const uint8_t* __restrict__ k_new, const uint8_t* __restrict__ v_new,
                                                        int64_t sb, int64_t sh, int64_t st, int Hkv, int T, int nbr,
                                                        int64_t nblocks, uint8_t* __restrict__ k_cache, uint8_t* __restrict__ v_cache,
                                                        int64_t S_cap, int64_t pos0) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x, blk = id >> 1;
    const int h = (int)(id & 1);
    if (blk >= nblocks) return;  // (both lanes of a block take the same side: the exchange below is between active lanes)
    const uint8_t* x = blockIdx.y ? v_new : k_new;
    uint8_t* cache = blockIdx.y ? v_cache : k_cache;
    const int j = (int)(blk % nbr);
    const int64_t row = blk / nbr;  // (b * Hkv + head) * T + t
    const int t = (int)(row % T);
    const int64_t bh = row / T, b = bh / Hkv, head = bh - b * Hkv;
    const uint4* p = reinterpret_cast<const uint4*>(x + (b * sb + head * sh + t * st + 32 * j + 16 * h) * 2);
    const uint4 w[2] = {p[0], p[1]};
    float v[16];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const uint32_t u[4] = {w[q].x, w[q].y, w[q].z, w[q].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint16_t lo = (uint16_t)(u[i] & 0xffffu), hi = (uint16_t)(u[i] >> 16);
            v[8 * q + 2 * i] = BF16 ? bf2f(lo) : h2f(lo);
            v[8 * q + 2 * i + 1] = BF16 ? bf2f(hi) : h2f(hi);
        }
    }
    float amax = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k) amax = fmaxf(amax, fabsf(v[k]));
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    const float d = amax / 127.0f;
    const float idv = d != 0.0f ? 1.0f / d : 0.0f;
    uint16_t* ob = reinterpret_cast<uint16_t*>(cache + ((bh * S_cap + pos0 + t) * nbr + j) * 34);
    if (h == 0) ob[0] = f2h(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int q0 = (int)roundf(v[2 * k] * idv), q1 = (int)roundf(v[2 * k + 1] * idv);
        ob[1 + 8 * h + k] = (uint16_t)((uint32_t)(q0 & 0xff) | ((uint32_t)(q1 & 0xff) << 8));
    }
}

}  // namespace

// the checks the two entry points of the cache share (the layout of gptq_gguf_kvcache.h): everything about x_dtype, B, Hkv, T,
// D, S_cap, pos0 and the strides of a [B, H, T, D] operand
int check_kv_shape(const char* who, int x_dtype, int64_t B, int64_t Hkv, int64_t T, int64_t D, int64_t S_cap, int64_t pos0) {
    if (x_dtype != GQ_F16 && x_dtype != GQ_BF16) GQ_FAIL(GQ_E_BAD_TYPE, "%s: x_dtype %d (GQ_F16 or GQ_BF16)", who, x_dtype);
    if (D != 64 && D != 128) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: D=%ld (64 or 128)", who, (long)D);
    if (B < 1 || Hkv < 1 || T < 1) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: B=%ld Hkv=%ld T=%ld (each at least 1)", who, (long)B, (long)Hkv, (long)T);
    if (S_cap < 4 || S_cap % 4 || B > 0x7fffffff / Hkv || B * Hkv > 0x7fffffff / S_cap)
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: S_cap=%ld (S_cap %% 4 != 0, or B * Hkv * S_cap not below 2^31)", who, (long)S_cap);
    if (pos0 < 0 || T > S_cap || pos0 > S_cap - T)
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: pos0=%ld + T=%ld > S_cap=%ld", who, (long)pos0, (long)T, (long)S_cap);
    return GQ_OK;
}
int check_kv_strides(const char* who, const char* name, int64_t sb, int64_t sh, int64_t st) {
    if (sb < 0 || sh < 0 || st < 0 || (sb | sh | st) % 8)
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: strides of %s (%ld, %ld, %ld) must be non-negative multiples of 8 elements", who, name, (long)sb,
                (long)sh, (long)st);
    return GQ_OK;
}

}  // namespace gq

using namespace gq;
using namespace gq::blockdec;

extern "C" {

int gq_kv_append_q8_0(const void* k_new, const void* v_new, int x_dtype, int64_t new_sb, int64_t new_sh, int64_t new_st, int64_t B,
                      int64_t Hkv, int64_t T, int64_t D, uint8_t* k_cache, uint8_t* v_cache, int64_t S_cap, int64_t pos0,
                      void* stream) {
    if (int rc = options_ok()) return rc;
    const char* who = "gq_kv_append_q8_0";
    if (int rc = check_kv_shape(who, x_dtype, B, Hkv, T, D, S_cap, pos0)) return rc;
    if (int rc = need(who, "k_new", k_new)) return rc;
    if (int rc = need(who, "v_new", v_new)) return rc;
    if (int rc = need(who, "k_cache", k_cache)) return rc;
    if (int rc = need(who, "v_cache", v_cache)) return rc;
    if (int rc = check_kv_strides(who, "k_new / v_new", new_sb, new_sh, new_st)) return rc;
    if (int rc = check_aligned(who, "k_new", k_new, 16)) return rc;
    if (int rc = check_aligned(who, "v_new", v_new, 16)) return rc;
    if (int rc = check_aligned(who, "k_cache", k_cache, 16)) return rc;
    if (int rc = check_aligned(who, "v_cache", v_cache, 16)) return rc;
    const int nbr = (int)(D / 32);
    const int64_t nblocks = B * Hkv * T * nbr;  // < 2^31 * 4
    const dim3 grid((unsigned)((2 * nblocks + 255) / 256), 2);
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* kp = static_cast<const uint8_t*>(k_new);
    const uint8_t* vp = static_cast<const uint8_t*>(v_new);
    dispatch_bool(x_dtype == GQ_BF16, [&](auto bf16) {
        hipLaunchKernelGGL((kv_append_kernel<decltype(bf16)::value>), grid, dim3(256), 0, st, kp, vp, new_sb, new_sh, new_st, (int)Hkv,
                           (int)T, nbr, nblocks, k_cache, v_cache, S_cap, pos0);
    });
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
