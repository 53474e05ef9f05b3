// gq_attn_plan.hpp -- the pure plan of one gq_attn_decode_q8_0 call (K33, attn/gq_attn_decode.hip): how the S = pos0 + T
// positions of the cache are cut into chunks, one workgroup per (chunk, column tile, KV head, batch row), and the workspace the
// partial results need.  Host arithmetic only, no HIP header: the launcher, gq_attn_decode_q8_0_workspace_bytes,
// gq_attn_decode_q8_0_plan and tests/attn_plan_dump.cpp all read this one text.  The plan is a function of (S, B, Hkv, tiles)
// and the constants below -- the CU count is the MI355X's, a constant as SYRK_CUS is, not a query of the device --, so a shape
// has one split on every machine and its result is the same bits on every call.
#pragma once

#include <cstddef>
#include <cstdint>

namespace gq {

constexpr int ATTN_TILE = 16;        // (g, t) columns of a workgroup: the N of one MFMA
constexpr int ATTN_MAX_COLS = 64;    // GQ_ATTN_DECODE_MAX_COLS
constexpr int ATTN_NW = 4;           // waves of a workgroup
constexpr int ATTN_SUB = 32;         // positions of a wave's sub-chunk: one K step of the P V MFMA, a multiple of 4 rows = 16 bytes
constexpr int ATTN_TURN = ATTN_NW * ATTN_SUB;  // positions a workgroup takes per turn of its loop
constexpr int ATTN_MIN_CHUNK = 2 * ATTN_TURN;  // a shorter cache is not split: a chunk amortises the q fragment and the merge
constexpr int ATTN_MAX_SPLITS = 64;  // chunks of a call at most (the merge kernel walks them serially)
constexpr int ATTN_CUS = 256;        // MI355X
constexpr int ATTN_WGS_PER_CU = 2;   // workgroups the plan aims at: two per CU hide each other's softmax between the streams

struct AttnPlan {
    int64_t splits, chunk;  // chunk i is positions [i * chunk, min(S, (i + 1) * chunk)); chunk % ATTN_SUB == 0
    int tiles;
};

inline int attn_tiles(int64_t cols) { return (int)((cols + ATTN_TILE - 1) / ATTN_TILE); }

inline AttnPlan make_attn_plan(int64_t S, int64_t B, int64_t Hkv, int64_t cols) {
    AttnPlan p{};
    p.tiles = attn_tiles(cols);
    const int64_t base = B * Hkv * p.tiles;  // workgroups of an unsplit call
    int64_t want = (int64_t)ATTN_CUS * ATTN_WGS_PER_CU / base;
    const int64_t by_len = (S + ATTN_MIN_CHUNK - 1) / ATTN_MIN_CHUNK;
    if (want > by_len) want = by_len;
    if (want > ATTN_MAX_SPLITS) want = ATTN_MAX_SPLITS;
    if (want < 1) want = 1;
    const int64_t per = (S + want - 1) / want;
    p.chunk = (per + ATTN_SUB - 1) / ATTN_SUB * ATTN_SUB;
    p.splits = (S + p.chunk - 1) / p.chunk;  // (no empty chunk)
    return p;
}

// one partial per (batch row, KV head, tile, chunk): 16 columns of { O[D], m, l } in fp32
inline size_t attn_partial_floats(int64_t D) { return (size_t)ATTN_TILE * ((size_t)D + 2); }
inline size_t attn_workspace_bytes(int64_t S, int64_t B, int64_t Hkv, int64_t cols, int64_t D) {
    const AttnPlan p = make_attn_plan(S, B, Hkv, cols);
    return (size_t)B * (size_t)Hkv * (size_t)p.tiles * (size_t)p.splits * attn_partial_floats(D) * 4;
}

}  // namespace gq
