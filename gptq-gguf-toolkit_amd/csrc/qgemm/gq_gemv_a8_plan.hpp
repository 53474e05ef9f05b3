// gq_gemv_a8_plan.hpp -- the pure plan of one gq_gemv_packed_a8 call (K37, qgemm/gq_gemv_a8.hip): the LDS image of the
// quantized activations and whether it fits, the rows a workgroup takes per turn of its grid-stride loop, the cap of the
// grid and the grid.  Plain arithmetic, no HIP header: the launcher and gq_gemv_a8_plan read this one text.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GQ_A8_PLAN_FN __host__ __device__ inline
#else
#define GQ_A8_PLAN_FN inline
#endif

namespace gq {

constexpr int GEMV_A8_NW = 16;                  // waves of a workgroup: a wave owns one row per turn
constexpr int GEMV_A8_ROWS = GEMV_A8_NW;        // rows of a workgroup's turn
constexpr int GEMV_A8_LANES = 4;                // lanes that own one superblock of a row: 64 values each
constexpr int GEMV_A8_STEP = 64 / GEMV_A8_LANES;  // superblocks of a row that a wave takes per step
// One workgroup of 16 waves per CU (256 CUs): every workgroup quantizes x once, so more workgroups than CUs would repeat
// the prologue for nothing.
constexpr int64_t GEMV_A8_GRID_CAP = 256;
// The image must leave room for nothing else: the kernel has no other LDS.  128 KiB of the CU's 160.
constexpr int64_t GEMV_A8_LDS_BUDGET = 128 * 1024;

struct GemvA8Plan {
    int64_t lds_bytes;      // the image of T rows: codes T C, group sums of 16 as int16 T C / 8, fp32 steps T C / 64
    int64_t rows_per_turn;  // GEMV_A8_ROWS
    int64_t turns;          // row groups of the call: ceil(R / rows_per_turn)
    int64_t grid_cap;       // GEMV_A8_GRID_CAP
    int64_t grid;           // min(turns, grid_cap): workgroup b takes row groups b, b + grid, ...
    bool fits;              // lds_bytes <= GEMV_A8_LDS_BUDGET
};

// byte offsets of the three parts of the image (each a multiple of 16 for C % 256 == 0); the kernel reads these too
GQ_A8_PLAN_FN int64_t gemv_a8_off_bsum(int64_t T, int64_t C) { return T * C; }
GQ_A8_PLAN_FN int64_t gemv_a8_off_d(int64_t T, int64_t C) { return T * C + T * C / 8; }

// T >= 1, R >= 1, C % 256 == 0 (the caller has checked)
inline GemvA8Plan make_gemv_a8_plan(int64_t T, int64_t R, int64_t C) {
    GemvA8Plan p{};
    p.lds_bytes = gemv_a8_off_d(T, C) + T * C / 64;
    p.rows_per_turn = GEMV_A8_ROWS;
    p.turns = (R + GEMV_A8_ROWS - 1) / GEMV_A8_ROWS;
    p.grid_cap = GEMV_A8_GRID_CAP;
    p.grid = p.turns < p.grid_cap ? p.turns : p.grid_cap;
    p.fits = p.lds_bytes <= GEMV_A8_LDS_BUDGET;
    return p;
}

}  // namespace gq
