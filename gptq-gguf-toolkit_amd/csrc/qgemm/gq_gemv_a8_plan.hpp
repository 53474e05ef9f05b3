// gq_gemv_a8_plan.hpp -- the pure plan of one gq_gemv_packed_a8 call (K37, qgemm/gq_gemv_a8.hip): the LDS image of the
// quantized activations and whether it fits, the rows a workgroup takes per turn of its grid-stride loop, the cap of the
// grid and the grid; the same for one gq_gemv_packed_experts_a8 call (K38, qgemm/gq_moe_gemv_a8.hip); and the partition of the
// grid among the members of one gq_gemv_packed_group_a8 call (K39, qgemm/gq_gemv_group_a8.hip).  Plain arithmetic, no HIP
// header: the launchers, gq_gemv_a8_plan, gq_gemv_experts_a8_plan and gq_gemv_group_a8_plan read this one text.
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

// ---- gq_gemv_packed_experts_a8 (K38, qgemm/gq_moe_gemv_a8.hip): the grid is (grid_x, E) and only the workgroups of a hit
// expert work.  The host cannot know how many experts a step hits, so the cap is per expert: with two hit experts (Mixtral
// at T = 1) 128 is one workgroup per CU.  Measured against 64 and 256 in profiles/moe_gemv_a8_rate.txt (DESIGN K38).
#ifndef GQ_GEMV_EXPERTS_A8_GRID_X_CAP  // (the profile's A/B builds the library with another value)
#define GQ_GEMV_EXPERTS_A8_GRID_X_CAP 128
#endif
constexpr int64_t GEMV_EXPERTS_A8_GRID_X_CAP = GQ_GEMV_EXPERTS_A8_GRID_X_CAP;
constexpr int GEMV_EXPERTS_A8_PASS = 4;  // matching pairs of a pass: the tokens of one image
// The kernel switches per workgroup between the 1 .. 4-token instances of the row walk.  Defined (A/B builds only): one
// 4-token instance with idle columns instead, whose image always has 4 rows.
#ifdef GQ_GEMV_EXPERTS_A8_IDLE_COLUMNS
constexpr bool GEMV_EXPERTS_A8_IDLE_COLUMNS = true;
#else
constexpr bool GEMV_EXPERTS_A8_IDLE_COLUMNS = false;
#endif

struct GemvExpertsA8Plan {
    int64_t image_rows;     // min(P, GEMV_EXPERTS_A8_PASS): the most rows of x a pass quantizes
    int64_t lds_bytes;      // the image of image_rows rows (make_gemv_a8_plan's layout)
    int64_t rows_per_turn;  // GEMV_A8_ROWS
    int64_t grid_x_cap;     // GEMV_EXPERTS_A8_GRID_X_CAP
    int64_t grid_x;         // min(ceil(R / rows_per_turn), grid_x_cap): workgroup (b, e) takes row groups b, b + grid_x, ... of expert e
    bool fits;              // lds_bytes <= GEMV_A8_LDS_BUDGET
};

// P >= 1, R >= 1, C % 256 == 0 (the caller has checked)
inline GemvExpertsA8Plan make_gemv_experts_a8_plan(int64_t P, int64_t R, int64_t C) {
    GemvExpertsA8Plan p{};
    p.image_rows = P < GEMV_EXPERTS_A8_PASS && !GEMV_EXPERTS_A8_IDLE_COLUMNS ? P : GEMV_EXPERTS_A8_PASS;
    p.lds_bytes = gemv_a8_off_d(p.image_rows, C) + p.image_rows * C / 64;
    p.rows_per_turn = GEMV_A8_ROWS;
    p.grid_x_cap = GEMV_EXPERTS_A8_GRID_X_CAP;
    const int64_t turns = (R + GEMV_A8_ROWS - 1) / GEMV_A8_ROWS;
    p.grid_x = turns < p.grid_x_cap ? turns : p.grid_x_cap;
    p.fits = p.lds_bytes <= GEMV_A8_LDS_BUDGET;
    return p;
}

// ---- gq_gemv_packed_group_a8 (K39, qgemm/gq_gemv_group_a8.hip): up to GEMV_GROUP_A8_MAX weights of one input in one 1-D
// grid of at most GEMV_A8_GRID_CAP workgroups; member m owns workgroups [first_wg[m], first_wg[m + 1]) and its workgroup b
// walks the member's row groups b - first_wg[m], + its count, ..  The partition, by largest remainder on the weight bytes:
//   cap_m   = ceil(R_m / GEMV_A8_ROWS)                        a member cannot use more workgroups than it has row groups
//   grid    = min(GEMV_A8_GRID_CAP, sum cap_m)
//   quota_m = grid * bytes_m / sum bytes,  bytes_m = R_m * row_bytes_m           (a rational; compared exactly, in integers)
//   g_m     = min(max(floor(quota_m), 1), cap_m)
//   while sum g_m < grid: one more to the member with g_m < cap_m whose quota_m - g_m is largest (a tie: the lowest m)
//   while sum g_m > grid: one less for the member with g_m > 1 whose quota_m - g_m is smallest (a tie: the highest m)
// (the second loop runs only where the floor of 1 lifted a tiny member).  Both loops end: grid <= sum cap_m and grid >= n.
// In SWIGLU mode the two members (equal R, equal type) share every workgroup: a wave walks gate row r and up row r back to
// back, so the grid is min(GEMV_A8_GRID_CAP, cap_0) and first_wg = {0, 0, grid}.
constexpr int GEMV_GROUP_A8_MAX = 4;

struct GemvGroupA8Plan {
    int64_t lds_bytes;                        // make_gemv_a8_plan's image of T rows
    int64_t grid;                             // workgroups of the launch
    int64_t first_wg[GEMV_GROUP_A8_MAX + 1];  // [0 .. n]: member m's first workgroup; first_wg[n] = grid
    bool fits;                                // lds_bytes <= GEMV_A8_LDS_BUDGET
};

// 1 <= n <= GEMV_GROUP_A8_MAX, T >= 1, every R >= 1 and row_bytes >= 1, C % 256 == 0 (the caller has checked)
inline GemvGroupA8Plan make_gemv_group_a8_plan(const int64_t* R, const int64_t* row_bytes, int n, int64_t C, int64_t T, bool swiglu) {
    GemvGroupA8Plan p{};
    p.lds_bytes = gemv_a8_off_d(T, C) + T * C / 64;
    p.fits = p.lds_bytes <= GEMV_A8_LDS_BUDGET;
    int64_t cap[GEMV_GROUP_A8_MAX], g[GEMV_GROUP_A8_MAX], sum_cap = 0;
    for (int m = 0; m < n; ++m) sum_cap += cap[m] = (R[m] + GEMV_A8_ROWS - 1) / GEMV_A8_ROWS;
    if (swiglu) {
        p.grid = cap[0] < GEMV_A8_GRID_CAP ? cap[0] : GEMV_A8_GRID_CAP;
        p.first_wg[0] = p.first_wg[1] = 0, p.first_wg[2] = p.grid;
        return p;
    }
    typedef __int128 wide;  // grid * bytes_m reaches 2^70 at the largest R and C the call takes
    p.grid = sum_cap < GEMV_A8_GRID_CAP ? sum_cap : GEMV_A8_GRID_CAP;
    wide total = 0;
    for (int m = 0; m < n; ++m) total += (wide)R[m] * row_bytes[m];
    // rem(m) = (quota_m - g_m) * total
    auto rem = [&](int m) { return (wide)p.grid * R[m] * row_bytes[m] - (wide)g[m] * total; };
    int64_t sum = 0;
    for (int m = 0; m < n; ++m) {
        const int64_t fl = (int64_t)((wide)p.grid * R[m] * row_bytes[m] / total);
        sum += g[m] = fl < 1 ? 1 : fl > cap[m] ? cap[m] : fl;
    }
    for (; sum < p.grid; ++sum) {
        int best = -1;
        for (int m = 0; m < n; ++m)
            if (g[m] < cap[m] && (best < 0 || rem(m) > rem(best))) best = m;
        ++g[best];
    }
    for (; sum > p.grid; --sum) {
        int best = -1;
        for (int m = n - 1; m >= 0; --m)
            if (g[m] > 1 && (best < 0 || rem(m) < rem(best))) best = m;
        --g[best];
    }
    for (int m = 0; m < n; ++m) p.first_wg[m + 1] = p.first_wg[m] + g[m];
    return p;
}

}  // namespace gq
