// gq_gemv_a8.hip -- K37: the decode step of a packed model on int8 activations.
//   gq_gemv_packed_a8  y = x W^T for 1 <= T <= 4 tokens: x is quantized to the Q8 activation format inside the kernel and
//                      multiplied with the integer codes of the packed weight on the VALU's 4 x int8 dot product
//   gq_gemv_a8_plan    the LDS image, the rows of a turn, the grid: csrc/qgemm/gq_gemv_a8_plan.hpp
// The contract is include/gptq_gguf_qgemv_a8.h's.  No weight becomes a float and no matrix instruction is issued: at T <= 4
// an MFMA tile is at least three quarters empty, while v_dot4_i32_i8 does four multiply-adds per lane and needs only the
// shifts and masks that turn the stored bits into bytes.
//
// Prologue.  A workgroup of 16 waves quantizes the T rows of x once into LDS with a8core::quantize_superblock -- the text
// gq_quantize_act_q8 runs, so the image [codes T C | group sums of 16, int16, T C / 8 | steps, fp32, T C / 64] is byte for
// byte what that call writes -- 32 superblocks per pass.  The grid is capped at one workgroup per CU and a workgroup walks row
// groups b, b + grid, .. so that lm_head's > 100 k rows pay for 256 prologues, not 8000.  A wave issues the loads of its
// first row BEFORE the prologue; the barrier after the prologue is the only one of the kernel.
//
// Work split.  A wave owns one row per turn (16 rows per workgroup and turn) and all of C: no K split across waves, no LDS
// reduction.  Four lanes own one superblock of the row, 64 values each, so the 64 lanes of a wave cover 16 consecutive
// superblocks = one contiguous run of the row's bytes per step (all of a 4096-column row at once).  A lane loads its piece of
// the block STRAIGHT INTO REGISTERS (no LDS staging of weights), unpacks it once into sixteen 4 x int8 operands and reuses
// them for every token against xq read from LDS (ds_read_b128, 64 bytes per token).  The next step's pieces are in flight
// while this one's dot products run.  What a lane holds of superblock j, lane p = 0 .. 3 of its group:
//   Q4_K / Q5_K  the 64-value chunk p: qs[32 p .. + 31] (Q5_K: and all of qh), i.e. groups 2 p and 2 p + 1 whole; the 16
//                header bytes in every lane (one address per group: a broadcast)
//   Q2_K / Q3_K / Q6_K  half ch = p >> 1 of the superblock, bytes l0 = 16 (p & 1) .. + 15 of its 32-byte planes: quarter k of
//                those bytes is the whole 16-value group 8 ch + 2 k + (p & 1), values 128 ch + 32 k + l0 .. + 15
//   Q8_0         blocks 2 p and 2 p + 1, 68 contiguous bytes: two d and two runs of 32 codes
// so every lane holds whole scale groups: a group's products are summed by four (eight) dot4, multiplied by the integer
// scale and added up in the lane; isum and msum = sum mn_g xbsum_g are then reduced over the four lanes AS INTEGERS (two
// exchanges each) -- exact.  Every lane of the group computes the contract's fp32 sequence xd (d float(isum) - dmin float(msum))
// (Q8_0: d_b float(isum_b) per block, summed pairwise over the eight blocks) and adds it to its accumulator of that token; at
// the end of the row the sixteen lane groups are summed by a binary tree of exchanges and lane t stores token t, rounded once.
//
// 2-byte aligned types (Q3_K 110 B, Q6_K 210 B, Q8_0 8 x 34 B).  A piece of n dwords at a 2-byte aligned address a with
// a % 4 == 2 is fetched as [2 bytes at a][n - 1 aligned dwords from a + 2][2 bytes at a + 4 n - 2] and put together with
// v_alignbyte; with a % 4 == 0 it is n aligned dwords.  Exactly the piece's bytes either way: nothing before the first block
// or after the last is touched, wherever the buffer begins.  (K22: 14 - 34 two-byte loads per lane and superblock.)
#include "../../../include/gptq_gguf_qgemv_a8.h"

#include <atomic>

#include "../search/gq_block_host.hpp"
#include "gq_gemv_a8_plan.hpp"
#include "gq_qgemm_a8_core.hpp"

namespace gq {
namespace {

using namespace a8core;  // quantize_superblock, signed4, A8<QT>; through it blockdec's loads and layouts

typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));  // four dwords at a 4-byte aligned address

constexpr int NT = 64 * GEMV_A8_NW;
constexpr uint32_t M01 = 0x01010101u, M03 = 0x03030303u, M0F = 0x0f0f0f0fu;

// registers of a lane's share of one superblock, as loaded
template <int QT> constexpr int NRAW = QT == GQ_Q2_K ? 7 : QT == GQ_Q3_K ? 12 : QT == GQ_Q4_K ? 12 : QT == GQ_Q5_K ? 20 : QT == GQ_Q6_K ? 15 : 17;
// bytes of a row's share of one superblock
template <int QT> constexpr int ROWB = QL<QT>::ROWB;

__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int c) { return __builtin_amdgcn_sdot4((int)a, (int)b, c, false); }

// N dwords from a (a - s is 4-byte aligned, s = 0 or 2): see the head of the file
template <int N>
__device__ __forceinline__ void piece(const uint8_t* a, uint32_t s, uint32_t* w) {
    const uint8_t* q = a - s;
    uint32_t d[N + 1];
    d[0] = s ? (uint32_t)ld2(a) << 16 : ld4(a);
#pragma unroll
    for (int i = 1; i < N; ++i) d[i] = ld4(q + 4 * i);
    d[N] = s ? (uint32_t)ld2(q + 4 * N) : 0u;
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], s);
}

// lane p's share of the superblock at A
template <int QT>
__device__ __forceinline__ void load_raw(const uint8_t* A, int p, uint32_t* w) {
    const int ch = p >> 1, l0 = 16 * (p & 1);
    const uint32_t s = (uint32_t)reinterpret_cast<uintptr_t>(A) & 2u;  // every piece begins at a multiple of 4 from A
    if constexpr (QT == GQ_Q4_K) {  // {d, dmin, scales[12]} | qs[32 p .. + 31]
        ld16(A, w), ld16(A + 16 + 32 * p, w + 4), ld16(A + 32 + 32 * p, w + 8);
    } else if constexpr (QT == GQ_Q5_K) {  // header | qh[32] | qs[32 p .. + 31]
        ld16(A, w), ld16(A + 16, w + 4), ld16(A + 32, w + 8), ld16(A + 48 + 32 * p, w + 12), ld16(A + 64 + 32 * p, w + 16);
    } else if constexpr (QT == GQ_Q2_K) {  // qs[32 ch + l0 .. + 15] | scales[8 ch .. + 7] | {d, dmin}
        const u32x4a4 v = *reinterpret_cast<const u32x4a4*>(A + 16 + 16 * p);
        w[0] = v[0], w[1] = v[1], w[2] = v[2], w[3] = v[3];
        w[4] = ld4(A + 8 * ch), w[5] = ld4(A + 8 * ch + 4), w[6] = ld4(A + 80);
    } else if constexpr (QT == GQ_Q3_K) {  // qs[32 ch + l0 .. + 15] | hmask[l0 .. + 15] | scales[12] | d
        piece<4>(A + 32 + 16 * p, s, w), piece<4>(A + l0, s, w + 4), piece<3>(A + 96, s, w + 8);
        w[11] = ld2(A + 108);
    } else if constexpr (QT == GQ_Q6_K) {  // ql[64 ch + l0 ..] | ql[64 ch + 32 + l0 ..] | qh[32 ch + l0 ..] | scales[8 ch .. + 7] | d
        piece<4>(A + 64 * ch + l0, s, w), piece<4>(A + 64 * ch + 32 + l0, s, w + 4), piece<4>(A + 128 + 16 * p, s, w + 8);
        piece<2>(A + 192 + 8 * ch, s, w + 12);
        w[14] = ld2(A + 208);
    } else {  // Q8_0: blocks 2 p and 2 p + 1 as they lie, {d, qs[32]} {d, qs[32]}
        piece<17>(A + 68 * p, s, w);
    }
}

__device__ __forceinline__ u32x4 lds16(const int8_t* p) { return *reinterpret_cast<const u32x4*>(p); }
__device__ __forceinline__ int dot16(const uint32_t* c, u32x4 x, int acc) {
    return dot4(c[3], x[3], dot4(c[2], x[2], dot4(c[1], x[1], dot4(c[0], x[0], acc))));
}

// The integer part of a lane for superblock j and TT tokens: w as loaded, X = the image's codes at superblock j of token 0
// (token t at X + t C), BS = the image's group sums at superblock j of token 0 (token t at BS + t C / 16).
// K-quants: isum[t], msum[t] of the lane's groups and (d, dmin); Q8_0: fs[t] = d_b float(isum_b) summed over the lane's two blocks.
template <int QT, int TT>
__device__ __forceinline__ void lane_dots(const uint32_t* w, int p, const int8_t* X, const int16_t* BS, int C, int* isum, int* msum,
                                          float* fs, float& d, float& dmin) {
    const int ch = p >> 1, hb = p & 1, l0 = 16 * hb;
    uint32_t c[16];  // the lane's 64 codes as int8 operands: c[4 k + i] = bytes 4 i .. 4 i + 3 of its k-th run of 16
    int sc[4], mn[4] = {0, 0, 0, 0};
    d = dmin = 0.f;
    if constexpr (QT == GQ_Q4_K || QT == GQ_Q5_K) {  // runs 0, 1: group 2 p; runs 2, 3: group 2 p + 1
        const uint32_t* q = w + (QT == GQ_Q5_K ? 12 : 4);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            c[i] = q[i] & M0F, c[8 + i] = (q[i] >> 4) & M0F;
            if constexpr (QT == GQ_Q5_K) c[i] |= ((w[4 + i] >> (2 * p)) & M01) << 4, c[8 + i] |= ((w[4 + i] >> (2 * p + 1)) & M01) << 4;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {  // get_scale_min_k4 on the 12 scale bytes (group_scale's text, from registers)
            const int g = 2 * p + u, sh = 8 * (g & 3);
            const int s6 = (w[1] >> sh) & 63, m6 = (w[2] >> sh) & 63;
            const int s4 = ((w[3] >> sh) & 0xF) | (((w[1] >> (sh + 6)) & 3) << 4), m4 = ((w[3] >> (sh + 4)) & 0xF) | (((w[2] >> (sh + 6)) & 3) << 4);
            sc[u] = g < 4 ? s6 : s4, mn[u] = g < 4 ? m6 : m4;
        }
        d = h2f((uint16_t)w[0]), dmin = h2f((uint16_t)(w[0] >> 16));
    } else if constexpr (QT == GQ_Q8_0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], 2), c[8 + i] = w[9 + i];
    } else {  // run k = quarter k of the lane's 16 plane bytes = group 8 ch + 2 k + hb
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int bsh = 8 * (2 * (k & 1) + hb);  // the group's byte within its scale word
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (QT == GQ_Q2_K) c[4 * k + i] = (w[i] >> (2 * k)) & M03;
                else if constexpr (QT == GQ_Q3_K) c[4 * k + i] = signed4<QT>(((w[i] >> (2 * k)) & M03) | (((w[4 + i] >> (4 * ch + k)) & M01) << 2));
                else c[4 * k + i] = signed4<QT>(((w[4 * (k & 1) + i] >> (4 * (k >> 1))) & M0F) | (((w[8 + i] >> (2 * k)) & M03) << 4));
            }
            if constexpr (QT == GQ_Q2_K) {
                const uint32_t v = (w[4 + (k >> 1)] >> bsh) & 0xffu;
                sc[k] = v & 0xF, mn[k] = v >> 4;
            } else if constexpr (QT == GQ_Q3_K) {  // six bits: a nibble of scales[0 .. 7], two bits of scales[8 .. 11]
                const uint32_t lo = (w[8 + (k >> 1)] >> (bsh + 4 * ch)) & 0xF, hi = (w[10] >> (bsh + 2 * (2 * ch + (k >> 1)))) & 3;
                sc[k] = (int)(lo | (hi << 4)) - 32;
            } else {
                sc[k] = (int)(int8_t)(w[12 + (k >> 1)] >> bsh);
            }
        }
        if constexpr (QT == GQ_Q2_K) d = h2f((uint16_t)w[6]), dmin = h2f((uint16_t)(w[6] >> 16));
        else d = h2f((uint16_t)w[QT == GQ_Q3_K ? 11 : 14]);
    }
#pragma unroll
    for (int t = 0; t < TT; ++t) {
        const int8_t* Xt = X + t * C;
        if constexpr (A8<QT>::G32) {  // 64 contiguous codes of the token
            const int a = dot16(c + 4, lds16(Xt + 64 * p + 16), dot16(c, lds16(Xt + 64 * p), 0));
            const int b = dot16(c + 12, lds16(Xt + 64 * p + 48), dot16(c + 8, lds16(Xt + 64 * p + 32), 0));
            if constexpr (QT == GQ_Q8_0) {
                fs[t] = h2f((uint16_t)w[0]) * (float)a + h2f((uint16_t)(w[8] >> 16)) * (float)b;
            } else {
                const uint2 bs = *reinterpret_cast<const uint2*>(BS + t * (C / 16) + 4 * p);  // the sums of the lane's four 16s
                isum[t] = sc[0] * a + sc[1] * b;
                msum[t] = mn[0] * ((int)(int16_t)bs.x + (int)(int16_t)(bs.x >> 16)) + mn[1] * ((int)(int16_t)bs.y + (int)(int16_t)(bs.y >> 16));
            }
        } else {
            int is = 0, ms = 0;
            u32x4 bs = {0u, 0u, 0u, 0u};
            if constexpr (QT == GQ_Q2_K) bs = *reinterpret_cast<const u32x4*>(BS + t * (C / 16) + 8 * ch);  // groups 8 ch .. + 7
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                is += sc[k] * dot16(c + 4 * k, lds16(Xt + 128 * ch + 32 * k + l0), 0);
                if constexpr (QT == GQ_Q2_K) ms += mn[k] * (int)(int16_t)(bs[k] >> (16 * hb));
            }
            isum[t] = is, msum[t] = ms;
        }
    }
}

template <int QT, int TT>
__global__ __launch_bounds__(NT) void gemv_packed_a8_kernel(const uint8_t* __restrict__ blocks, const int32_t* __restrict__ row_src,
                                                           int64_t R, int C, const uint16_t* __restrict__ x, int bf16,
                                                           uint16_t* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) uint8_t a8_img[];
    constexpr int NW = NRAW<QT>;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), p = lane & 3, g4 = lane >> 2;
    const int nsb = C / 256, nsteps = (nsb + GEMV_A8_STEP - 1) / GEMV_A8_STEP;
    int8_t* sxq = reinterpret_cast<int8_t*>(a8_img);
    int16_t* sbs = reinterpret_cast<int16_t*>(a8_img + gemv_a8_off_bsum(TT, C));
    float* sxd = reinterpret_cast<float*>(a8_img + gemv_a8_off_d(TT, C));

    // lane group g4's superblock of step `st` of row r (r < R), if the row has one
    auto load_item = [&](uint32_t* w, int64_t r, int st) {
        const int j = GEMV_A8_STEP * st + g4;
        if (j < nsb) load_raw<QT>(blocks + ((row_src ? (int64_t)row_src[r] : r) * nsb + j) * ROWB<QT>, p, w);
    };

    int64_t r = (int64_t)blockIdx.x * GEMV_A8_ROWS + wave;
    int step = 0;
    uint32_t cur[NW] = {};
    if (r < R) load_item(cur, r, 0);  // in flight during the prologue

    // ---- the prologue: x -> the image, 32 superblocks per pass
    const int tot = TT * nsb;
    for (int s0 = 0; s0 < tot; s0 += NT / 32) {
        const int sbi = s0 + (tid >> 5), piece8 = tid & 31;
        const bool on = sbi < tot;  // (a whole half wave is on or off)
        uint4 raw = make_uint4(0, 0, 0, 0);
        if (on) raw = *reinterpret_cast<const uint4*>(x + (int64_t)sbi * 256 + piece8 * 8);
        const uint32_t xw[4] = {raw.x, raw.y, raw.z, raw.w};
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint16_t b = (uint16_t)(xw[k >> 1] >> (16 * (k & 1)));
            v[k] = bf16 ? bf2f(b) : h2f(b);
        }
        quantize_superblock(v, on, sbi, piece8, sxq, sxd, sbs);
    }
    __syncthreads();

    float facc[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) facc[t] = 0.f;
#pragma unroll 1
    while (r < R) {
        int nstep = step + 1;
        int64_t nr = r;
        if (nstep == nsteps) nstep = 0, nr = r + (int64_t)gridDim.x * GEMV_A8_ROWS;
        uint32_t nxt[NW] = {};
        if (nr < R) load_item(nxt, nr, nstep);

        const int j = GEMV_A8_STEP * step + g4;
        const bool active = j < nsb;
        const int jc = active ? j : 0;  // (an idle lane group reads superblock 0 of the image and drops the result)
        int isum[TT], msum[TT];
        float fs[TT], d, dmin;
        lane_dots<QT, TT>(cur, p, sxq + 256 * jc, sbs + 16 * jc, C, isum, msum, fs, d, dmin);
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            float v;
            if constexpr (QT == GQ_Q8_0) {
                v = fs[t];
                v += __shfl_xor(v, 1);
                v += __shfl_xor(v, 2);
            } else {
                int is = isum[t];
                is += __shfl_xor(is, 1);
                is += __shfl_xor(is, 2);
                v = d * (float)is;
                if constexpr (A8<QT>::MINS) {
                    int ms = msum[t];
                    ms += __shfl_xor(ms, 1);
                    ms += __shfl_xor(ms, 2);
                    v = v - dmin * (float)ms;
                }
            }
            const float term = sxd[t * nsb + jc] * v;
            facc[t] += active ? term : 0.f;
        }

        if (step == nsteps - 1) {  // the row is complete: the sixteen lane groups, then one rounding
#pragma unroll
            for (int t = 0; t < TT; ++t) {
                float v = facc[t];
#pragma unroll
                for (int m = GEMV_A8_LANES; m < 64; m <<= 1) v += __shfl_xor(v, m);
                if (lane == t) y[(int64_t)t * R + r] = bf16 ? f2bf(v) : f2h(v);
                facc[t] = 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) cur[i] = nxt[i];
        r = nr, step = nstep;
    }
}

template <int QT, int TT>
int launch(const GemvA8Plan& pl, const uint8_t* blocks, const int32_t* row_src, int64_t R, int64_t C, const uint16_t* x, int bf16,
           uint16_t* y, hipStream_t st) {
    static std::atomic<bool> attr_set{false};
    if (!attr_set) {
        GQ_HIP(hipFuncSetAttribute((const void*)gemv_packed_a8_kernel<QT, TT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)GEMV_A8_LDS_BUDGET));
        attr_set = true;
    }
    hipLaunchKernelGGL((gemv_packed_a8_kernel<QT, TT>), dim3((unsigned)pl.grid), dim3(NT), (size_t)pl.lds_bytes, st, blocks, row_src, R,
                       (int)C, x, bf16, y);
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_gemv_a8_plan(int64_t T, int64_t R, int64_t C, int64_t* lds_bytes, int64_t* rows_per_turn, int64_t* grid_cap, int64_t* grid,
                    int64_t* fits) {
    const char* who = "gq_gemv_a8_plan";
    if (T < 1 || T > GQ_GEMV_A8_MAX_T) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: T=%ld (not in [1, %d])", who, (long)T, GQ_GEMV_A8_MAX_T);
    if (int rc = check_R(who, R)) return rc;
    if (int rc = check_C256(who, C)) return rc;
    const GemvA8Plan p = make_gemv_a8_plan(T, R, C);
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    if (rows_per_turn) *rows_per_turn = p.rows_per_turn;
    if (grid_cap) *grid_cap = p.grid_cap;
    if (grid) *grid = p.grid;
    if (fits) *fits = p.fits;
    return GQ_OK;
}

int gq_gemv_packed_a8(int q_type, const void* blocks, const int32_t* row_src, int64_t R, int64_t C, const void* x, int64_t T,
                      int x_dtype, void* y, void* stream) {
    if (int rc = options_ok()) return rc;
    const char* who = "gq_gemv_packed_a8";
    if (q_type == GQ_IQ4_NL || q_type == GQ_IQ4_XS)
        GQ_FAIL(GQ_E_BAD_TYPE, "%s: q_type %d (%s) is not served on int8 activations (a K-quant or GQ_Q8_0)", who, q_type,
                q_type == GQ_IQ4_NL ? "GQ_IQ4_NL" : "GQ_IQ4_XS");
    if (!a8_type(q_type)) GQ_FAIL(GQ_E_BAD_TYPE, "%s: unknown q_type %d (a K-quant or GQ_Q8_0)", who, q_type);
    if (int rc = check_types(who, q_type, x_dtype)) return rc;
    if (int rc = need(who, "blocks", blocks)) return rc;
    if (int rc = need(who, "x", x)) return rc;
    if (int rc = need(who, "y", y)) return rc;
    if (int rc = check_R(who, R)) return rc;
    if (T < 1 || T > GQ_GEMV_A8_MAX_T)
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: T=%ld (not in [1, %d]; gq_gemv_packed takes up to %d tokens)", who, (long)T, GQ_GEMV_A8_MAX_T,
                GQ_GEMV_MAX_T);
    if (int rc = check_C256(who, C)) return rc;
    const GemvA8Plan pl = make_gemv_a8_plan(T, R, C);
    if (!pl.fits)
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: T=%ld C=%ld: the quantized image of x, %ld bytes, does not fit the %ld bytes of LDS it may take",
                who, (long)T, (long)C, (long)pl.lds_bytes, (long)GEMV_A8_LDS_BUDGET);
    if (int rc = check_blocks_aligned(who, q_type, blocks)) return rc;
    if (int rc = check_aligned(who, "row_src", row_src, 4)) return rc;
    if (int rc = check_aligned(who, "x", x, 16)) return rc;
    if (int rc = check_aligned(who, "y", y, 16)) return rc;
    int rc = GQ_OK;
    dispatch_packed(q_type, [&](auto qt) {
        constexpr int QT = decltype(qt)::value;
        if constexpr (a8_type(QT)) {
            auto go = [&](auto tt) {
                rc = launch<QT, decltype(tt)::value>(pl, static_cast<const uint8_t*>(blocks), row_src, R, C, static_cast<const uint16_t*>(x),
                                                     (int)(x_dtype == GQ_BF16), static_cast<uint16_t*>(y), (hipStream_t)stream);
            };
            switch (T) {
            case 1: go(std::integral_constant<int, 1>{}); break;
            case 2: go(std::integral_constant<int, 2>{}); break;
            case 3: go(std::integral_constant<int, 3>{}); break;
            default: go(std::integral_constant<int, 4>{}); break;
            }
        }
    });
    return rc;
}

}  // extern "C"
