// gq_attn_prefill.hip -- K34: the attention of MANY query tokens over a KV cache kept as Q8_0 blocks
// (include/gptq_gguf_kvprefill.h): a chunk of a long prompt, or a later turn of a conversation, at positions pos0 .. pos0 + T - 1
// over the pos0 + T rows of the cache.  gq_attn_decode_q8_0 (K33) stops at 64 columns per KV head because each of its waves
// decodes the packed bytes for its own 16 columns; here a packed byte is decoded ONCE PER WORKGROUP into a 16-bit image in LDS
// that all the waves read as MFMA operands, so the decode amortises over the 64 columns of the workgroup.
//
// One launch, no workspace, no atomics.  The grid is one-dimensional, gq_attn_prefill_plan.hpp's: a workgroup of 4 waves owns one
// (batch row, KV head) and one block of 64 columns c = t G + g (token t, query head h G + g), 16 per wave, and walks the
// positions in turns of 32 from the turn of kv_start[b] to the turn of its last token's position: nothing is split over
// workgroups, so nothing is merged, and the blocks of early tokens stop early.  The last blocks walk longest and are launched
// first.  A wave skips the arithmetic of a turn that lies wholly past its own last token (it still stages and decodes).
//
// A turn.  (1) The packed K rows and V rows of the turn are each one 16-byte aligned run of 32 * RB bytes (RB = 68 / 136);
// they were fetched with 16-byte loads during the previous turn's arithmetic and go from registers to a raw LDS region with
// 16-byte stores.  (2) After a barrier the next turn's loads are issued, and the 256 threads decode the raw bytes co-operatively:
// a thread takes half a block (one d, 16 codes read as 2-byte LDS loads, the packed stream being 2-byte aligned) and writes 16
// values of 16 bits -- q8_0_dequantize1 + cvt_out, the bits of gq_dequantize_blocks -- with two 16-byte stores into the K or V
// image, [32 positions][D + 8] elements: the pad of 16 bytes turns the 16 rows of a 16-byte read onto distinct banks.  The d of
// a position below kv_start[b] or past pos0 + T - 1 is replaced by 0: such a row decodes to zeros whatever its bytes are.
// (3) After a second barrier every wave computes from the images; the next turn's stage follows the first barrier of that turn,
// so raw region and images are single buffers.
//
// Q K^T is K33's: v_mfma_f32_16x16x32_{f16,bf16}, A = 16 positions x 32 head-dim values of K, one 16-byte LDS read per lane
// (lane (r = l & 15, u = l >> 4): values 32 kb + 8 u .. + 7 of position r), B = the q fragment held in registers for the whole
// walk, result S[4 u + i][c = l & 15].  Scale, mask by select, online softmax in fp32 per column as there.
//
// P V: O^T[dim][c] += V^T[dim][pos] P[pos][c] with K33's naming of the contraction index (k = 8 u + j is position 4 u + j of
// the first score tile or 16 + 4 u + j - 4 of the second: the lane's own probabilities are its B operand) and of the output row
// (row m of tile mt is dim NT m + mt, NT = D / 16).  The V operand: for each of its 8 positions a lane reads the NT consecutive
// 16-bit values NT (l & 15) .. of the V image row -- ONE 16-byte (D = 128) or 8-byte (D = 64) LDS read per position -- and
// builds the operand of tile mt by taking element mt of the eight reads: a register transpose of 16-bit halves, one byte
// permute per operand dword (4 per MFMA).  DESIGN K34 compares this with the transpose reads.
//
// A column that saw nothing (its token lies below kv_start[b]) ends with l = 0 and is written as exact zeros.
#include "../../../include/gptq_gguf_kvprefill.h"

#include "../qgemm/gq_gemv_core.hpp"  // mfma<BF16>, the vector types
#include "../search/gq_block_host.hpp"
#include "gq_attn_prefill_plan.hpp"

namespace gq {

// attn/gq_kv_append.hip: the checks of the cache's layout
int check_kv_shape(const char* who, int x_dtype, int64_t B, int64_t Hkv, int64_t T, int64_t D, int64_t S_cap, int64_t pos0);
int check_kv_strides(const char* who, const char* name, int64_t sb, int64_t sh, int64_t st);

namespace {

using namespace gemvcore;

constexpr float NEG_INF = -__builtin_inff();
constexpr int NTHR = 64 * PREFILL_NW;

// e^x for x <= 0 (and -inf -> 0): v_exp_f32 on x log2(e)
__device__ __forceinline__ float fexp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

template <typename OutT>
__device__ __forceinline__ uint32_t pack2(float a, float b) {
    return (uint32_t)cvt_out<OutT>(a).b | ((uint32_t)cvt_out<OutT>(b).b << 16);
}

// the low / high 16-bit halves of two dwords as one dword, a's in the low half: one v_perm_b32 each (selector bytes 0 .. 3
// name the bytes of the builtin's second operand, 4 .. 7 those of its first)
__device__ __forceinline__ uint32_t lo_halves(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x05040100u); }
__device__ __forceinline__ uint32_t hi_halves(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }

template <int D> struct PrefillGeo {
    static constexpr int NKB = D / 32, RB = NKB * 34, NT = D / 16;
    static constexpr int RAWB = PREFILL_TURN * RB;               // packed bytes of a turn of K (and of V)
    static constexpr int NLD = (RAWB / 16 + NTHR - 1) / NTHR;    // 16-byte loads per thread and cache
    static constexpr int PITCH = (D + 8) * 2;                    // bytes of an image row
    static constexpr int IMGB = PREFILL_TURN * PITCH;            // bytes of an image
    static constexpr int UNITS = 2 * PREFILL_TURN * NKB * 2;     // half blocks of a turn: K and V
    static constexpr int LDS = 2 * RAWB + 2 * IMGB;
    static_assert(RAWB % 16 == 0 && PITCH % 16 == 0 && UNITS % NTHR == 0, "16-byte pieces; whole rounds of the decode");
};

template <int D, bool BF16>
__global__ __launch_bounds__(NTHR) void attn_prefill_kernel(const uint8_t* __restrict__ q, int64_t q_sb, int64_t q_sh, int64_t q_st,
                                                            const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
                                                            int64_t S_cap, int pos0, int T, int G, int B, int Hkv, int64_t blocks,
                                                            const int32_t* __restrict__ kv_start, float scale,
                                                            uint16_t* __restrict__ out) {
    using OutT = typename std::conditional<BF16, bf16_bits, half_bits>::type;
    using A = PrefillGeo<D>;
    constexpr int NKB = A::NKB, RB = A::RB, NT = A::NT, NLD = A::NLD, PITCH = A::PITCH;
    __shared__ __attribute__((aligned(16))) uint8_t smem[A::LDS];
    uint8_t* const raw = smem;                      // K rows, then V rows, as they lie in the cache
    uint8_t* const kimg = smem + 2 * A::RAWB;       // [32][D + 8] 16-bit
    uint8_t* const vimg = kimg + A::IMGB;
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, u = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const PrefillWho who = prefill_who(blockIdx.x, blocks, B, Hkv);
    const int b = (int)who.b, h = (int)who.h;
    const int64_t cols = (int64_t)G * T, cb = who.block * PREFILL_COLS;
    const int S = pos0 + T;
    int start = kv_start ? kv_start[b] : 0;
    start = start < 0 ? 0 : start;

    // the lane's column: token t, query head h G + g; a column past G T carries zeros, sees no position and is not written
    const int64_t col = cb + PREFILL_WAVE_COLS * wave + l15;
    const bool on = col < cols;
    const int t = on ? (int)(col / G) : 0, g = on ? (int)(col - (int64_t)t * G) : 0;
    const int last = on ? pos0 + t : -1;
    u32x4 qf[NKB];
    const uint8_t* qp = q + ((int64_t)b * q_sb + (int64_t)(h * G + g) * q_sh + (int64_t)t * q_st + 8 * u) * 2;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) qf[kb] = on ? *reinterpret_cast<const u32x4*>(qp + 64 * kb) : u32x4{0, 0, 0, 0};

    // the walk of the block, and the last position any column of this wave sees (wave-uniform)
    const int blast = pos0 + (int)prefill_last_token(who.block, T, G);
    const int64_t wc = cb + PREFILL_WAVE_COLS * wave;
    int wlast = -1;
    if (wc < cols) {
        const int64_t we = wc + PREFILL_WAVE_COLS - 1 < cols - 1 ? wc + PREFILL_WAVE_COLS - 1 : cols - 1;
        wlast = pos0 + (int)(we / G);
    }
    wlast = __builtin_amdgcn_readfirstlane(wlast);
    const int turn0 = start / PREFILL_TURN, turn1 = blast / PREFILL_TURN;  // turn1 < turn0, or start > blast in it: nothing seen

    const int64_t slab = ((int64_t)b * Hkv + h) * S_cap * RB;
    const uint8_t* kg = kc + slab;
    const uint8_t* vg = vc + slab;

    f32x4 o[NT];
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) o[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = NEG_INF, l = 0.f;

    u32x4 pk[NLD] = {}, pv[NLD] = {};
    const auto prefetch = [&](int turn) {  // the rows [p0, min(p0 + 32, S)) of both caches, 16 bytes per thread and round
        const int p0 = turn * PREFILL_TURN, n = ((S - p0) < PREFILL_TURN ? (S - p0) : PREFILL_TURN) * RB;
        const int64_t off = (int64_t)p0 * RB;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int at = (tid + NTHR * i) * 16;
            if (at < n) {  // (the last load may reach past row S - 1; it stays inside the slab because S_cap % 4 == 0)
                pk[i] = *reinterpret_cast<const u32x4*>(kg + off + at);
                pv[i] = *reinterpret_cast<const u32x4*>(vg + off + at);
            }
        }
    };
    if (turn0 <= turn1) prefetch(turn0);
#pragma unroll 1
    for (int turn = turn0; turn <= turn1; ++turn) {
        const int p0 = turn * PREFILL_TURN;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int at = (tid + NTHR * i) * 16;
            if (at < A::RAWB) {
                *reinterpret_cast<u32x4*>(raw + at) = pk[i];
                *reinterpret_cast<u32x4*>(raw + A::RAWB + at) = pv[i];
            }
        }
        __syncthreads();  // the raw rows are in place; every wave has left the images of the previous turn
        if (turn < turn1) prefetch(turn + 1);  // in flight during this turn's decode and arithmetic

        // the co-operative decode: unit e = (((kv * 32 + r) * NKB + kb) * 2 + half), 16 values each
#pragma unroll
        for (int e = tid; e < A::UNITS; e += NTHR) {
            const int hf = e & 1, blk = e >> 1, kb = blk % NKB, r = (blk / NKB) % PREFILL_TURN, kv = blk / (NKB * PREFILL_TURN);
            const uint8_t* src = raw + kv * A::RAWB + r * RB + 34 * kb;
            const int p = p0 + r;
            const float d = (p >= start && p < S) ? h2f(ld2(src)) : 0.f;
            uint32_t w[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint32_t two = (p < S) ? ld2(src + 2 + 16 * hf + 2 * i) : 0u;  // (stale bytes are finite codes anyway)
                w[i] = pack2<OutT>(q8_0_dequantize1(d, two & 0xffu), q8_0_dequantize1(d, two >> 8));
            }
            uint8_t* dst = (kv ? vimg : kimg) + r * PITCH + (32 * kb + 16 * hf) * 2;
            *reinterpret_cast<u32x4*>(dst) = u32x4{w[0], w[1], w[2], w[3]};
            *reinterpret_cast<u32x4*>(dst + 16) = u32x4{w[4], w[5], w[6], w[7]};
        }
        __syncthreads();  // the images are whole; the raw region may be overwritten
        if (p0 > wlast) continue;  // the turn lies wholly past this wave's columns (wave-uniform; no barrier below)

        // scores of the two tiles of 16 positions
        float sv[8];
        float mx = NEG_INF;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const uint8_t* row = kimg + (16 * a + l15) * PITCH + 16 * u;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) acc = mfma<BF16>(*reinterpret_cast<const u32x4*>(row + 64 * kb), qf[kb], acc);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int p = p0 + 16 * a + 4 * u + i;
                const bool seen = p >= start && p <= last;
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

        // the V fragment: dims NT l15 .. NT l15 + NT - 1 of the lane's 8 positions, one LDS read per position
        constexpr int NW = NT / 2;  // dwords of a read
        uint32_t vr[8][NW];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int prow = j < 4 ? 4 * u + j : 16 + 4 * u + (j - 4);
            const uint8_t* r = vimg + prow * PITCH + NT * l15 * 2;
            if constexpr (NT == 8) {
                const u32x4 x = *reinterpret_cast<const u32x4*>(r);
                vr[j][0] = x[0], vr[j][1] = x[1], vr[j][2] = x[2], vr[j][3] = x[3];
            } else {
                const uint2 x = *reinterpret_cast<const uint2*>(r);
                vr[j][0] = x.x, vr[j][1] = x.y;
            }
        }
#pragma unroll
        for (int mt = 0; mt < NT; ++mt) {
            u32x4 av;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                av[jj] = (mt & 1) ? hi_halves(vr[2 * jj][mt >> 1], vr[2 * jj + 1][mt >> 1]) : lo_halves(vr[2 * jj][mt >> 1], vr[2 * jj + 1][mt >> 1]);
            o[mt] = mfma<BF16>(av, pf, o[mt]);
        }
    }

    // normalise and round once: lane (c = l15, u) holds dims NT (4 u + i) + mt of its column
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (!on) return;
    const float inv = l > 0.f ? 1.f / l : 0.f;  // a column that saw nothing: O = 0 and l = 0 -> exact zeros
    const int64_t Hq = (int64_t)Hkv * G;
    uint16_t* po = out + (((int64_t)b * T + t) * Hq + (int64_t)h * G + g) * D;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t w[NT / 2];
#pragma unroll
        for (int e = 0; e < NT / 2; ++e)
            w[e] = pack2<OutT>(o[2 * e][i] * inv, o[2 * e + 1][i] * inv);
        uint16_t* p = po + NT * (4 * u + i);
        if constexpr (NT == 8) *reinterpret_cast<u32x4*>(p) = u32x4{w[0], w[1], w[2], w[3]};
        else *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
    }
}

}  // namespace
}  // namespace gq

using namespace gq;
using namespace gq::blockdec;

extern "C" {

int gq_attn_prefill_q8_0_plan(int64_t T, int64_t G, int64_t* block_cols, int64_t* turn, int64_t* blocks) {
    if (T < 1 || G < 1 || G > 0x7fffffff / T)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_attn_prefill_q8_0_plan: T=%ld G=%ld (each at least 1, G*T below 2^31)", (long)T, (long)G);
    if (block_cols) *block_cols = PREFILL_COLS;
    if (turn) *turn = PREFILL_TURN;
    if (blocks) *blocks = make_prefill_plan(T, G, 1, 1).blocks;
    return GQ_OK;
}

int gq_attn_prefill_q8_0(const void* q, int x_dtype, int64_t q_sb, int64_t q_sh, int64_t q_st, int64_t B, int64_t Hq, int64_t Hkv,
                         int64_t T, int64_t D, const uint8_t* k_cache, const uint8_t* v_cache, int64_t S_cap, int64_t pos0,
                         const int32_t* kv_start, float scale, void* out, void* stream) {
    if (int rc = options_ok()) return rc;
    const char* who = "gq_attn_prefill_q8_0";
    if (int rc = check_kv_shape(who, x_dtype, B, Hkv, T, D, S_cap, pos0)) return rc;
    if (Hq < Hkv || Hq % Hkv) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: Hq=%ld is not a multiple of Hkv=%ld", who, (long)Hq, (long)Hkv);
    const int64_t G = Hq / Hkv;
    if (G > 0x7fffffff / T) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: G*T=%ld*%ld (not below 2^31)", who, (long)G, (long)T);
    const PrefillPlan p = make_prefill_plan(T, G, B, Hkv);  // (B * Hkv < 2^31 by check_kv_shape, blocks < 2^25: no overflow)
    if (p.grid > 0x7fffffff)
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: %ld column blocks * B=%ld * Hkv=%ld workgroups (not below 2^31)", who, (long)p.blocks, (long)B, (long)Hkv);
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

    hipStream_t st = (hipStream_t)stream;
    const uint8_t* qp = static_cast<const uint8_t*>(q);
    uint16_t* op = static_cast<uint16_t*>(out);
    dispatch_bool(D == 128, [&](auto wide) {
        dispatch_bool(x_dtype == GQ_BF16, [&](auto bf16) {
            constexpr int DD = decltype(wide)::value ? 128 : 64;
            constexpr bool BF = decltype(bf16)::value;
            hipLaunchKernelGGL((attn_prefill_kernel<DD, BF>), dim3((unsigned)p.grid), dim3(NTHR), 0, st, qp, q_sb, q_sh, q_st, k_cache,
                               v_cache, S_cap, (int)pos0, (int)T, (int)G, (int)B, (int)Hkv, p.blocks, kv_start, scale, op);
        });
    });
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // extern "C"
