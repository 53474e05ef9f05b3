// gq_attn_prefill_plan.hpp -- the pure plan of one gq_attn_prefill_q8_0 call (K34, attn/gq_attn_prefill.hip): how the G T
// query columns c = t G + g of a KV head are cut into blocks, one workgroup per (column block, batch row, KV head), the turn
// of positions a workgroup takes per step of its walk, and the order of the workgroups in the one-dimensional grid.  Host
// arithmetic only, no HIP header: the launcher and gq_attn_prefill_q8_0_plan read this one text, and the kernel undoes the
// grid order with the same function.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GQ_PLAN_FN __host__ __device__ inline
#else
#define GQ_PLAN_FN inline
#endif

namespace gq {

constexpr int PREFILL_NW = 4;                                // waves of a workgroup
constexpr int PREFILL_WAVE_COLS = 16;                        // columns of a wave: the N of one MFMA
constexpr int PREFILL_COLS = PREFILL_NW * PREFILL_WAVE_COLS; // columns of a workgroup
constexpr int PREFILL_TURN = 32;                             // positions of a turn: the K of the P V MFMA, 16-byte aligned runs

struct PrefillPlan {
    int64_t blocks;  // column blocks of a (batch row, KV head): ceil(G T / PREFILL_COLS)
    int64_t grid;    // workgroups of the call: blocks * B * Hkv
};

inline PrefillPlan make_prefill_plan(int64_t T, int64_t G, int64_t B, int64_t Hkv) {
    PrefillPlan p{};
    p.blocks = (G * T + PREFILL_COLS - 1) / PREFILL_COLS;
    p.grid = p.blocks * B * Hkv;
    return p;
}

// Grid order: the walk of a column block ends at its last token's position, so the LAST block walks longest.  Workgroups are
// dispatched by rising index; index 0 .. B Hkv - 1 are the last column block of every (b, h), and so on down to block 0, whose
// short walks fill the tail.
struct PrefillWho {
    int64_t block, b, h;
};
GQ_PLAN_FN PrefillWho prefill_who(int64_t index, int64_t blocks, int64_t B, int64_t Hkv) {
    const int64_t bh = index % (B * Hkv);
    return {blocks - 1 - index / (B * Hkv), bh / Hkv, bh % Hkv};
}

// the turns [first, last] a block walks: from the turn of the first visible position to the turn of the position of its last
// token.  last < first: the block sees nothing (all of its tokens lie below kv_start).
GQ_PLAN_FN int64_t prefill_last_token(int64_t block, int64_t T, int64_t G) {
    const int64_t c = (block + 1) * PREFILL_COLS - 1, t = c / G;
    return t < T - 1 ? t : T - 1;
}

}  // namespace gq
