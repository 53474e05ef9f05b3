// gq_attn_decode.hip -- K33: the attention of a decode step over a KV cache kept as Q8_0 blocks (include/gptq_gguf_kvcache.h):
// out[b, hq, t] = softmax(scale q[b, hq, t] K[b, hq / G, 0 .. pos0 + t]^T) V for the T query tokens at positions pos0 .. pos0 +
// T - 1.  At T = 1 the call is one stream over the cache bytes, the regime of K22; the cache is read at its stored size, 34
// bytes per 32 values, and never exists in 16 bits.
//
// Split-KV, two launches, no atomics.  Grid (splits, column tiles * Hkv, B), the split being gq_attn_plan.hpp's.  A workgroup
// of 4 waves owns one KV head, one tile of <= 16 columns c = t G + g (query head h G + g, token t) and one chunk of positions.
// The G query heads of a group are columns of the same MFMA, so every K / V byte is read once for all of them (K22 puts the
// tokens there).  Wave w takes the sub-chunks w, w + 4, ... of 32 positions and keeps its own running (m, l, O) per column in
// registers; after the loop the four partials meet in LDS and are merged in wave order into ONE fp32 partial per column --
// running max m, sum l, unnormalised O[D] -- in the caller's workspace.  attn_merge_kernel (one workgroup of D threads per
// column) merges the splits in split order, normalises and rounds once.
//
// Staging.  A sub-chunk's packed rows are one contiguous run of 32 * RB bytes (RB = 68 / 136 bytes per row) that starts 16-byte
// aligned in its (b, h) slab -- chunks and sub-chunks start on multiples of 32 positions --, so it goes to the wave's own LDS
// region as it lies, with 16-byte loads and 16-byte LDS stores, consecutive lanes on consecutive 16 bytes (K22 staged Q8_0 2
// bytes at a time).  The loads of sub-chunk i + 4 are issued before the arithmetic of sub-chunk i and wait in registers; the
// LDS regions are wave-private, ordered by wavefront-scope fences, and no workgroup barrier sits in the loop.  The last 16-byte
// load of a chunk may reach past the chunk's last row; it stays inside the slab because S_cap % 4 == 0.
//
// Q K^T: v_mfma_f32_16x16x32_{f16,bf16} with A = 16 positions x the 32 values of ONE Q8_0 block of their K rows and B = 16
// columns x the same 32 head-dim values of q (held in registers for the whole chunk): lane (r = l & 15, u = l >> 4) decodes
// the 8 codes 8 u .. 8 u + 7 of position r's block with blockdec's q8_0_dequantize1 and cvt_out -- the operand bits are
// gq_dequantize_blocks' -- and receives S[4 u + i][c = l & 15] in register i.  The codes of a block lie 2-byte aligned in the
// packed stream, so they are read as 2-byte LDS loads.  Scores are scaled in fp32; a masked position (below kv_start[b], past
// pos0 + t, or past the end of the chunk) is set to -inf by a select, so whatever the bytes behind the last row decode to never
// reaches the running max.  The softmax is the online one in fp32, per column: the column's max over a sub-chunk is the max
// over the lane's 8 scores and two cross-lane exchanges (lanes c, c + 16, c + 32, c + 48 hold a column).
//
// P V: O^T[dim][c] += V^T[dim][pos] P[pos][c], 32 positions per MFMA.  The contraction index of an MFMA is free to name, and
// so is the output row: k = 8 u + j stands for position 4 u + j of the first score tile (j < 4) or 16 + 4 u + j - 4 of the
// second, which is exactly where the lane's own probabilities lie -- P goes from the score registers to the B operand with no
// exchange --, and output row m of dim tile mt stands for dim NT m + mt (NT = D / 16 tiles), so the NT bytes a lane needs of one
// V row for all its tiles are contiguous: the V fragment is a per-lane gather of NT bytes and one d for each of its 8
// positions, decoded cvt(d * q) with one rounding as the decoder does (DESIGN K33 says why not the transpose reads).  The d of
// a position past the chunk's end is replaced by 0, so that row contributes exactly zero whatever its bytes are.  P is rounded
// to the activation dtype for this MFMA; l sums the unrounded values.
#include "../../../include/gptq_gguf_kvcache.h"

#include "../qgemm/gq_gemv_core.hpp"  // mfma<BF16>, wave_sync, the vector types
#include "../search/gq_block_host.hpp"
#include "gq_attn_plan.hpp"

namespace gq {

// attn/gq_kv_append.hip: the checks of the cache's layout
int check_kv_shape(const char* who, int x_dtype, int64_t B, int64_t Hkv, int64_t T, int64_t D, int64_t S_cap, int64_t pos0);
int check_kv_strides(const char* who, const char* name, int64_t sb, int64_t sh, int64_t st);

namespace {

using namespace gemvcore;

constexpr float NEG_INF = -__builtin_inff();

// e^x for x <= 0 (and -inf -> 0): v_exp_f32 on x log2(e)
__device__ __forceinline__ float fexp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

template <typename OutT>
__device__ __forceinline__ uint32_t pack2(float a, float b) {
    return (uint32_t)cvt_out<OutT>(a).b | ((uint32_t)cvt_out<OutT>(b).b << 16);
}

template <int D> struct AttnGeo {
    static constexpr int NKB = D / 32, RB = NKB * 34, NT = D / 16;
    static constexpr int SUBB = ATTN_SUB * RB;          // bytes of a sub-chunk of K (and of V)
    static constexpr int NLD = (SUBB / 16 + 63) / 64;   // 16-byte loads per lane
    static constexpr int WAVE_LDS = 2 * SUBB;           // a wave's region: K rows, then V rows
    static constexpr int PF = ATTN_TILE * (D + 2);      // floats of a partial: O[16][D], m[16], l[16]
    static_assert(SUBB % 16 == 0 && PF * 4 <= WAVE_LDS, "a wave's region holds its partial");
};

template <int D, bool BF16>
__global__ __launch_bounds__(64 * ATTN_NW) void attn_decode_kernel(const uint8_t* __restrict__ q, int64_t q_sb, int64_t q_sh, int64_t q_st,
                                                                   const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
                                                                   int64_t S_cap, int pos0, int T, int G, int Hkv, int tiles, int chunk,
                                                                   const int32_t* __restrict__ kv_start, float scale,
                                                                   float* __restrict__ ws) {
    using OutT = typename std::conditional<BF16, bf16_bits, half_bits>::type;
    using A = AttnGeo<D>;
    constexpr int NKB = A::NKB, RB = A::RB, NT = A::NT, NLD = A::NLD;
    __shared__ __attribute__((aligned(16))) uint8_t smem[ATTN_NW * A::WAVE_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, u = lane >> 4;
    const int split = blockIdx.x, ti = blockIdx.y % tiles, h = blockIdx.y / tiles, b = blockIdx.z;
    const int S = pos0 + T, c0 = split * chunk, c1 = S - c0 < chunk ? S : c0 + chunk;
    const int start = kv_start ? kv_start[b] : 0;

    // the lane's column: token t, query head h G + g; a column past G T carries zeros and sees no position
    const int col = ATTN_TILE * ti + l15;
    const bool on = col < G * T;
    const int t = on ? col / G : 0, g = on ? col - t * G : 0;
    const int last = on ? pos0 + t : -1;
    u32x4 qf[NKB];
    const uint8_t* qp = q + ((int64_t)b * q_sb + (int64_t)(h * G + g) * q_sh + (int64_t)t * q_st + 8 * u) * 2;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) qf[kb] = on ? *reinterpret_cast<const u32x4*>(qp + 64 * kb) : u32x4{0, 0, 0, 0};

    const int64_t slab = ((int64_t)b * Hkv + h) * S_cap * RB;
    const uint8_t* kg = kc + slab;
    const uint8_t* vg = vc + slab;
    uint8_t* kl = smem + wave * A::WAVE_LDS;
    uint8_t* vl = kl + A::SUBB;

    f32x4 o[NT];
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) o[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = NEG_INF, l = 0.f;

    const int nsub = (c1 - c0 + ATTN_SUB - 1) / ATTN_SUB;
    u32x4 pk[NLD] = {}, pv[NLD] = {};
    const auto prefetch = [&](int sc) {  // the rows [p0, min(p0 + 32, c1)) of both caches, 16 bytes per lane and turn
        const int p0 = c0 + sc * ATTN_SUB, n = ((c1 - p0) < ATTN_SUB ? (c1 - p0) : ATTN_SUB) * RB;
        const int64_t off = (int64_t)p0 * RB;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int at = (lane + 64 * i) * 16;
            if (at < n) {
                pk[i] = *reinterpret_cast<const u32x4*>(kg + off + at);
                pv[i] = *reinterpret_cast<const u32x4*>(vg + off + at);
            }
        }
    };
    if (wave < nsub) prefetch(wave);
#pragma unroll 1
    for (int sc = wave; sc < nsub; sc += ATTN_NW) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int at = (lane + 64 * i) * 16;
            if (at < A::SUBB) {
                *reinterpret_cast<u32x4*>(kl + at) = pk[i];
                *reinterpret_cast<u32x4*>(vl + at) = pv[i];
            }
        }
        wave_sync();
        if (sc + ATTN_NW < nsub) prefetch(sc + ATTN_NW);  // in flight during this sub-chunk's arithmetic
        const int p0 = c0 + sc * ATTN_SUB;

        // scores of the two tiles of 16 positions
        float sv[8];
        float mx = NEG_INF;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const uint8_t* row = kl + (16 * a + l15) * RB;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                const float d = h2f(ld2(row + 34 * kb));
                const uint8_t* c = row + 34 * kb + 2 + 8 * u;
                uint32_t w[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t two = ld2(c + 2 * i);
                    w[i] = pack2<OutT>(q8_0_dequantize1(d, two & 0xffu), q8_0_dequantize1(d, two >> 8));
                }
                acc = mfma<BF16>(u32x4{w[0], w[1], w[2], w[3]}, qf[kb], acc);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int p = p0 + 16 * a + 4 * u + i;
                const bool seen = p >= start && p <= last && p < c1;
                sv[4 * a + i] = seen ? acc[i] * scale : NEG_INF;
                mx = fmaxf(mx, sv[4 * a + i]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));

        // online softmax: a column that has seen nothing yet keeps m = -inf, and every exponent is then taken against 0
        const float mn = fmaxf(m, mx), mref = mn == NEG_INF ? 0.f : mn;
        const float alpha = fexp(m - mref);
        float pr[8], ps = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            pr[j] = fexp(sv[j] - mref);
            ps += pr[j];
        }
        l = l * alpha + ps;
        m = mn;
#pragma unroll
        for (int mt = 0; mt < NT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) o[mt][i] *= alpha;
        const u32x4 pf = {pack2<OutT>(pr[0], pr[1]), pack2<OutT>(pr[2], pr[3]), pack2<OutT>(pr[4], pr[5]), pack2<OutT>(pr[6], pr[7])};

        // the V fragment: dims NT l15 .. NT l15 + NT - 1 (inside one block) of the lane's 8 positions
        constexpr int NW4 = NT / 4;
        const int vblk = (NT * l15) >> 5, voff = (NT * l15) & 31;
        float dv[8];
        uint32_t vb[8][NW4];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int prow = j < 4 ? 4 * u + j : 16 + 4 * u + (j - 4);
            const uint8_t* r = vl + prow * RB + 34 * vblk;
            dv[j] = p0 + prow < c1 ? h2f(ld2(r)) : 0.f;
#pragma unroll
            for (int wd = 0; wd < NW4; ++wd)
                vb[j][wd] = (uint32_t)ld2(r + 2 + voff + 4 * wd) | ((uint32_t)ld2(r + 2 + voff + 4 * wd + 2) << 16);
        }
#pragma unroll
        for (int mt = 0; mt < NT; ++mt) {
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = q8_0_dequantize1(dv[j], (vb[j][mt >> 2] >> (8 * (mt & 3))) & 0xffu);
            const u32x4 av = {pack2<OutT>(x[0], x[1]), pack2<OutT>(x[2], x[3]), pack2<OutT>(x[4], x[5]), pack2<OutT>(x[6], x[7])};
            o[mt] = mfma<BF16>(av, pf, o[mt]);
        }
        wave_sync();  // the region may be overwritten
    }

    // the wave's partial to its own region: O[c][D], m[16], l[16]
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    float* pw = reinterpret_cast<float*>(kl);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int mt = 0; mt < NT; ++mt) pw[l15 * D + NT * (4 * u + i) + mt] = o[mt][i];
    if (u == 0) pw[ATTN_TILE * D + l15] = m, pw[ATTN_TILE * D + ATTN_TILE + l15] = l;
    __syncthreads();

    // the four partials in wave order -> the workgroup's partial: thread (c, part) takes NT dims of column c
    const int c = tid >> 4, part = tid & 15;
    float mw[ATTN_NW], ms = NEG_INF;
#pragma unroll
    for (int w = 0; w < ATTN_NW; ++w) {
        mw[w] = reinterpret_cast<const float*>(smem + w * A::WAVE_LDS)[ATTN_TILE * D + c];
        ms = fmaxf(ms, mw[w]);
    }
    const float mref = ms == NEG_INF ? 0.f : ms;
    float lt = 0.f, acc[NT];
#pragma unroll
    for (int e = 0; e < NT; ++e) acc[e] = 0.f;
#pragma unroll
    for (int w = 0; w < ATTN_NW; ++w) {
        const float* pwv = reinterpret_cast<const float*>(smem + w * A::WAVE_LDS);
        const float f = fexp(mw[w] - mref);
        lt += f * pwv[ATTN_TILE * D + ATTN_TILE + c];
#pragma unroll
        for (int e = 0; e < NT; ++e) acc[e] += f * pwv[c * D + NT * part + e];
    }
    float* pg = ws + ((((int64_t)b * Hkv + h) * tiles + ti) * gridDim.x + split) * A::PF;
#pragma unroll
    for (int e = 0; e < NT; ++e) pg[c * D + NT * part + e] = acc[e];
    if (part == 0) pg[ATTN_TILE * D + c] = ms, pg[ATTN_TILE * D + ATTN_TILE + c] = lt;
}

// One workgroup of D threads per column: the splits' partials in split order.  A split in which the column saw nothing has
// l = 0 and is skipped.
template <int D, bool BF16>
__global__ __launch_bounds__(D) void attn_merge_kernel(const float* __restrict__ ws, int splits, int tiles, int Hkv, int G, int T,
                                                       uint16_t* __restrict__ out) {
    using OutT = typename std::conditional<BF16, bf16_bits, half_bits>::type;
    constexpr int PF = AttnGeo<D>::PF;
    const int col = blockIdx.x, h = blockIdx.y, b = blockIdx.z, d = threadIdx.x;
    const int ti = col / ATTN_TILE, c = col % ATTN_TILE, t = col / G, g = col - t * G;
    const float* base = ws + (((int64_t)b * Hkv + h) * tiles + ti) * splits * PF;
    float ms = NEG_INF;
    for (int s = 0; s < splits; ++s)
        if (base[(int64_t)s * PF + ATTN_TILE * D + ATTN_TILE + c] > 0.f) ms = fmaxf(ms, base[(int64_t)s * PF + ATTN_TILE * D + c]);
    float lt = 0.f, acc = 0.f;
    for (int s = 0; s < splits; ++s) {
        const float* p = base + (int64_t)s * PF;
        const float ls = p[ATTN_TILE * D + ATTN_TILE + c];
        if (!(ls > 0.f)) continue;
        const float f = fexp(p[ATTN_TILE * D + c] - ms);
        lt += f * ls;
        acc += f * p[c * D + d];
    }
    const int64_t Hq = (int64_t)Hkv * G;
    out[(((int64_t)b * T + t) * Hq + (int64_t)h * G + g) * D + d] = cvt_out<OutT>(acc / lt).b;
}

bool attn_shape_ok(int64_t S, int64_t B, int64_t Hkv, int64_t cols, int64_t D) {
    return (D == 64 || D == 128) && S >= 1 && S <= 0x7fffffff && B >= 1 && B <= 65535 && Hkv >= 1 && cols >= 1 && cols <= ATTN_MAX_COLS &&
           Hkv * attn_tiles(cols) <= 65535;
}

}  // namespace
}  // namespace gq

using namespace gq;
using namespace gq::blockdec;

extern "C" {

size_t gq_attn_decode_q8_0_workspace_bytes(int64_t S, int64_t B, int64_t Hkv, int64_t cols, int64_t D) {
    return attn_shape_ok(S, B, Hkv, cols, D) ? attn_workspace_bytes(S, B, Hkv, cols, D) : 0;
}

int gq_attn_decode_q8_0_plan(int64_t S, int64_t B, int64_t Hkv, int64_t cols, int64_t* splits, int64_t* chunk, int64_t* min_chunk,
                             int64_t* turn) {
    if (!attn_shape_ok(S, B, Hkv, cols, 64))
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_attn_decode_q8_0_plan: S=%ld B=%ld Hkv=%ld G*T=%ld (G*T in [1, %d], B and Hkv * tiles at most 65535)",
                (long)S, (long)B, (long)Hkv, (long)cols, ATTN_MAX_COLS);
    const AttnPlan p = make_attn_plan(S, B, Hkv, cols);
    if (splits) *splits = p.splits;
    if (chunk) *chunk = p.chunk;
    if (min_chunk) *min_chunk = ATTN_MIN_CHUNK;
    if (turn) *turn = ATTN_TURN;
    return GQ_OK;
}

int gq_attn_decode_q8_0(const void* q, int x_dtype, int64_t q_sb, int64_t q_sh, int64_t q_st, int64_t B, int64_t Hq, int64_t Hkv,
                        int64_t T, int64_t D, const uint8_t* k_cache, const uint8_t* v_cache, int64_t S_cap, int64_t pos0,
                        const int32_t* kv_start, float scale, void* out, void* ws, size_t ws_bytes, void* stream) {
    static_assert(ATTN_MAX_COLS == GQ_ATTN_DECODE_MAX_COLS, "the header's cap is the plan's");
    if (int rc = options_ok()) return rc;
    const char* who = "gq_attn_decode_q8_0";
    if (int rc = check_kv_shape(who, x_dtype, B, Hkv, T, D, S_cap, pos0)) return rc;
    if (Hq < Hkv || Hq % Hkv) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: Hq=%ld is not a multiple of Hkv=%ld", who, (long)Hq, (long)Hkv);
    const int64_t G = Hq / Hkv, cols = G * T;
    if (G > ATTN_MAX_COLS || cols > ATTN_MAX_COLS)
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: G*T=%ld*%ld (more than %d columns; the prefill is not this kernel's)", who, (long)G, (long)T,
                ATTN_MAX_COLS);
    if (!attn_shape_ok(pos0 + T, B, Hkv, cols, D))
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: B=%ld Hkv=%ld (B and Hkv * tiles at most 65535)", who, (long)B, (long)Hkv);
    if (int rc = need(who, "q", q)) return rc;
    if (int rc = need(who, "k_cache", k_cache)) return rc;
    if (int rc = need(who, "v_cache", v_cache)) return rc;
    if (int rc = need(who, "out", out)) return rc;
    if (int rc = check_kv_strides(who, "q", q_sb, q_sh, q_st)) return rc;
    if (int rc = check_aligned(who, "q", q, 16)) return rc;
    if (int rc = check_aligned(who, "k_cache", k_cache, 16)) return rc;
    if (int rc = check_aligned(who, "v_cache", v_cache, 16)) return rc;
    if (int rc = check_aligned(who, "out", out, 16)) return rc;
    if (int rc = check_aligned(who, "kv_start", kv_start, 4)) return rc;
    const size_t wneed = attn_workspace_bytes(pos0 + T, B, Hkv, cols, D);
    if (!ws || ws_bytes < wneed) GQ_FAIL(GQ_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws ? ws_bytes : (size_t)0, wneed);
    if (int rc = check_aligned(who, "ws", ws, 16)) return rc;

    const AttnPlan p = make_attn_plan(pos0 + T, B, Hkv, cols);
    const dim3 grid((unsigned)p.splits, (unsigned)(p.tiles * Hkv), (unsigned)B), mgrid((unsigned)cols, (unsigned)Hkv, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* qp = static_cast<const uint8_t*>(q);
    float* wp = static_cast<float*>(ws);
    uint16_t* op = static_cast<uint16_t*>(out);
    dispatch_bool(D == 128, [&](auto wide) {
        dispatch_bool(x_dtype == GQ_BF16, [&](auto bf16) {
            constexpr int DD = decltype(wide)::value ? 128 : 64;
            constexpr bool BF = decltype(bf16)::value;
            hipLaunchKernelGGL((attn_decode_kernel<DD, BF>), grid, dim3(64 * ATTN_NW), 0, st, qp, q_sb, q_sh, q_st, k_cache, v_cache, S_cap,
                               (int)pos0, (int)T, (int)G, (int)Hkv, p.tiles, (int)p.chunk, kv_start, scale, wp);
            hipLaunchKernelGGL((attn_merge_kernel<DD, BF>), mgrid, dim3(DD), 0, st, wp, (int)p.splits, p.tiles, (int)Hkv, (int)G, (int)T, op);
        });
    });
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
