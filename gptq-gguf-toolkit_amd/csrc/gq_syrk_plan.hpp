// gq_syrk_plan.hpp -- the pure plan of one grouped 16-bit SYRK launch (K1, gq_hessian.hip): which kernel a
// problem takes, the tile table with its K-split and XCD deal, the layout of the workspace, and the bound that
// gq_workspace_bytes reports for it.  Host arithmetic only, no HIP header: syrk16_launch, h_accumulate_workspace_bytes and
// tests/syrk_plan_dump.cpp all read this one text.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace gq {

constexpr int HT = 128;           // output tile of syrk16_kernel, and the granularity of C
constexpr int BT = 256;           // output tile of the two ring kernels (syrk16_256e_kernel, syrk16_256w_kernel)
constexpr int SYRK_TURN = 128;    // tokens per turn of the 4-slot operand ring (four half-stages of 32): T is padded to it
constexpr int H_MAX_GROUP = 8;    // problems per grouped launch
constexpr int SYRK_GROUP = 32;    // consecutive tiles the 32 CUs of an XCD run at the same time out of one L2
constexpr int SYRK_XCDS = 8;
constexpr int SYRK_CUS = 256;     // one round of tiles
constexpr size_t SYRK_SPLIT_CAP = 512;       // K-split units of a launch, and partial-sum slots, at most
constexpr int64_t SYRK_SPLIT_MIN_T = 8192;   // only long token ranges are split (every part is at least 8 turns of the ring)
constexpr uint32_t SYRK_NONE = 0xffffffffu;  // empty table entry; aux word of a unit that is not split
constexpr int SYRK_BAR_WORDS = 16;           // rendezvous counters: [0..7] rounds, [8..15] checkpoints inside a tile
constexpr size_t SYRK_SLOT_BYTES = (size_t)BT * BT * 4;  // one partial-sum slot: a 256 x 256 fp32 tile

// The options a launch reads, taken ONCE per entry-point call (syrk_options, gq_hessian.hip): a gq_option_set from another
// thread cannot give one launch the tile order of one setting and the split of another.
struct SyrkOptions {
    bool image, nosplit;  // syrk_image, syrk_nosplit
    int gw;               // syrk_gw
    int64_t ck, wgs;      // syrk_ck, syrk_wgs
};

// 16-bit inputs with C % 256 == 0 and T % 128 == 0 are read in place (syrk16_256w_kernel): only the tile table
// needs scratch.  Everything else goes through the re-laid-out operand image.
inline bool syrk_in_place(int64_t T, int64_t C, const SyrkOptions& o) {
    return (C % BT == 0) && (T % SYRK_TURN == 0) && !o.image;
}
// the kernel a problem takes: 2 = 256x256 ring kernel reading X in place, 1 = 256x256 ring kernel on the re-laid-out
// image (T not a multiple of 128, or option syrk_image), 0 = 128x128 kernel on the image (C % 256 != 0)
inline int syrk_kind(int64_t T, int64_t C, const SyrkOptions& o) { return (C % BT) ? 0 : (syrk_in_place(T, C, o) ? 2 : 1); }

// K-split of the last (partial) round of tiles (syrk16_256w_kernel): partial-sum slots a problem may need.
// Only long token ranges are split; option syrk_nosplit disables it.
inline size_t syrk_partial_slots(int64_t T, size_t ntile, const SyrkOptions& o) {
    if (T < SYRK_SPLIT_MIN_T || o.nosplit) return 0;
    return 4 * ntile < SYRK_SPLIT_CAP ? 4 * ntile : SYRK_SPLIT_CAP;
}
inline int64_t syrk_padded_T(int64_t T) { return (T + SYRK_TURN - 1) / SYRK_TURN * SYRK_TURN; }  // whole turns of the ring

// What gq_workspace_bytes reports for one problem.  An upper BOUND of what make_syrk_plan lays out, per problem, so that
// the bounds of a group add up to at least what its launches carve whichever way the problems are sorted into launches
// (tests/test_syrk_plan_cpu.py checks that it dominates).  The terms, in the order of the upload:
constexpr size_t SYRK_TABLE_SLACK = 320;  // words: tl <= units + 255 (groups of 32 rounded up to 8 equal rows), + the pad word
constexpr size_t SYRK_BOUND_ALIGN = 256;  // rounding a pointer up to 256
inline size_t syrk_workspace_bytes(int64_t T, int64_t C, const SyrkOptions& o) {
    const size_t nt = (size_t)(C / BT);
    const size_t ntile = nt * (nt + 1) / 2;
    const size_t table = (ntile + SYRK_SPLIT_CAP + SYRK_TABLE_SLACK) * 4 * 2  // [table | aux], units <= ntile + the cap
                         + SYRK_SPLIT_CAP * 8                                 // reduce list: two words per split tile
                         + SYRK_BOUND_ALIGN                                   // the table's start
                         + (size_t)(T / SYRK_TURN + 2) * 8                    // block addresses: a block holds >= 128 tokens
                         + SYRK_BAR_WORDS * 4;                                // rendezvous counters
    if (syrk_in_place(T, C, o)) return table + syrk_partial_slots(T, ntile, o) * SYRK_SLOT_BYTES + SYRK_BOUND_ALIGN;
    return (size_t)C * (size_t)syrk_padded_T(T) * 2 + SYRK_BOUND_ALIGN + table;
}

struct SyrkShape {
    int64_t T, C, nseg;  // nseg <= 1: X is contiguous; else nseg separate blocks of T / nseg tokens each (kind 2 only)
};

constexpr int64_t SYRK_NO_WORD = -1;  // "no such part in the upload"

// Everything about one launch that follows from its shapes and the options, by arithmetic alone.  Byte offsets count
// from the 256-aligned workspace pointer the launch starts from, word indices into `words`.
struct SyrkPlan {
    struct Problem {
        int64_t Tp;                 // T in whole ring turns
        int nt, tile_begin;         // tiles per dimension; kind 0: first super-tile of the problem in the grid
        size_t img_off, img_bytes;  // operand image (kinds 0 and 1; img_bytes == 0: X is read in place)
        int hs_per_seg;             // half-stages (32 tokens) per separate block, 0: contiguous
        int64_t seg_word;           // the 2 * nseg words of its block addresses, left zero for the launch to fill
    } p[H_MAX_GROUP];
    int kind, m;
    int total_tiles;              // kind 0: super-tiles of the grid
    std::vector<uint32_t> words;  // the upload: [table | aux | reduce list | 16 rendezvous words | pad | block addresses]
    size_t tl;                    // words of the table, and of aux: 8 rows of per_xcd
    int per_xcd, sp, n_reduce;    // sp: K-split factor (1: none); n_reduce: tiles of the last partial round, when split
    int64_t aux_word, reduce_word, bar_word;
    int ck, nck;                  // SyrkGroup::ck, nck
    size_t img_end, table_off, partial_off, partial_bytes;  // images [0, img_end), table, partial sums (sp > 1)
    unsigned grid, block;
    size_t total;                 // what the launch advances the workspace pointer by
};

inline SyrkPlan make_syrk_plan(int kind, const SyrkShape* s, int m, const SyrkOptions& o) {
    SyrkPlan pl{};
    pl.kind = kind;
    pl.m = m;
    pl.sp = 1;
    pl.aux_word = pl.reduce_word = pl.bar_word = SYRK_NO_WORD;
    pl.block = kind == 1 ? 512 : 256;
    int tiles = 0;
    size_t at = 0;
    for (int k = 0; k < m; ++k) {
        SyrkPlan::Problem& p = pl.p[k];
        p.Tp = syrk_padded_T(s[k].T);
        p.nt = (int)(s[k].C / (kind ? BT : HT));
        p.tile_begin = tiles;
        p.seg_word = SYRK_NO_WORD;
        p.img_off = at;
        if (kind != 2) {
            p.img_bytes = (size_t)s[k].C * p.Tp * 2;
            at += (p.img_bytes + 255) & ~(size_t)255;
        }
        if (!kind) {
            const int ns = (p.nt + 7) / 8;  // 8x8 super-tiles per dimension
            tiles += ns * (ns + 1) / 2;
        }
    }
    pl.total_tiles = tiles;
    pl.img_end = pl.table_off = pl.total = at;
    if (!kind) {
        pl.grid = (unsigned)((tiles + 7) / 8 * 8 * 64);
        return pl;
    }
    // Balanced schedule: the valid (ti <= tj) tiles of all problems, enumerated super-tile by super-tile
    // (8 x 4 tiles share 12 operand panels), are cut into groups of 32 CONSECUTIVE tiles -- one group =
    // what the 32 CUs of an XCD run at the same time out of one L2 -- and the groups are dealt
    // round-robin to the 8 XCDs, so every XCD gets the same number of tiles (+-32) and no workgroup
    // exits early.  (An arithmetic id -> super-tile map leaves XCDs up to 30 % apart: diagonal
    // super-tiles are half empty.)
    std::vector<uint32_t> all;
    // (option syrk_gw: the super-tile's width in tiles, 32 / gw rows.  r06 A/B of the fabric traffic on random operands at
    // C = 14336, profiles/r06_syrk_traffic_ab.txt: 4 x 8 (r02-r05) 29.7 GB of L2-miss reads per launch, 1312 TFLOP/s; 2 x 16
    // 41.5 GB, 1283; 1 x 32 51.3 GB, 1269; 8 x 4 (default since r06) 26.5 GB, 1332 -- and 89.3 against 90.2 ms per bench
    // step in four alternating pairs.  Which tiles fall into the K-split round depends on the shape, so H moves within
    // K1's tolerance class.)
    const int gw = o.gw, gh = SYRK_GROUP / gw;
    for (int k = 0; k < m; ++k) {
        const int nt = pl.p[k].nt, nsc = (nt + gw - 1) / gw, nsr = (nt + gh - 1) / gh;
        for (int sI = 0; sI < nsr; ++sI)
            for (int sJ = (sI * gh) / gw; sJ < nsc; ++sJ)
                for (int slot = 0; slot < SYRK_GROUP; ++slot) {
                    const int ti = sI * gh + slot / gw, tj = sJ * gw + slot % gw;
                    if (ti < nt && tj < nt && ti <= tj) all.push_back((uint32_t)k << 24 | (uint32_t)ti << 12 | (uint32_t)tj);
                }
    }
    // K-split of the last, partial round (in-place kernel): 1596 tiles of a 14336-wide Hessian are 6.23 rounds
    // of 256 CUs, and the 7th round would run 60 tiles on 256 CUs for a whole tile time.  The R = N mod 256
    // tiles left after the full rounds are cut into s token ranges each, s minimising ceil(R s / 256) / s
    // (14336: s = 4, +0.25 instead of +1 round; 3 x 4096: R = 152, s = 3, +0.67 instead of +1); every unit
    // stores raw fp32 sums and syrk_reduce_kernel adds them in fixed order (deterministic).
    const size_t N = all.size(), full = (N / SYRK_CUS) * SYRK_CUS, R = N - full;
    int sp = 1;
    size_t cap_units = 0;
    bool can_split = kind == 2 && R > 0;
    for (int k = 0; k < m && can_split; ++k) {
        const size_t slots = syrk_partial_slots(pl.p[k].Tp, (size_t)pl.p[k].nt * (pl.p[k].nt + 1) / 2, o);
        if (slots == 0) can_split = false;
        cap_units += slots;
    }
    if (cap_units > SYRK_SPLIT_CAP) cap_units = SYRK_SPLIT_CAP;  // (measured, r04: 1024 -- s = 5 instead of 3 for the three 4096-wide inputs of a dense block, 1.6 rounds instead of 1.667 -- is 1-2 % SLOWER: partial-sum traffic and a longer reduce)
    if (can_split) {
        double best = 1.0;
        for (int c = 2; c <= 8 && R * c <= cap_units; ++c) {
            const double cost = (double)((R * c + SYRK_CUS - 1) / SYRK_CUS) / c;
            if (cost < best - 1e-9) { best = cost; sp = c; }
        }
    }
    // a unit is a tile, or one of the sp token ranges of a tile of the last round; unit u lies in group u / 32, and the
    // groups go round-robin to the XCD rows
    const size_t units = sp > 1 ? full + R * sp : N, ngroups = (units + SYRK_GROUP - 1) / SYRK_GROUP;
    const int per_xcd = (int)((ngroups + SYRK_XCDS - 1) / SYRK_XCDS) * SYRK_GROUP;
    const size_t tl = (size_t)SYRK_XCDS * per_xcd, n_rlist = sp > 1 ? 2 * R : 0;
    std::vector<uint32_t>& w = pl.words;
    w.assign(2 * tl + n_rlist, SYRK_NONE);  // [table | aux | reduce list]
    const auto put = [&](size_t u, uint32_t tile, uint32_t aux) {
        const size_t gi = u / SYRK_GROUP, pos = (gi % SYRK_XCDS) * per_xcd + (gi / SYRK_XCDS) * SYRK_GROUP + u % SYRK_GROUP;
        w[pos] = tile;
        w[tl + pos] = aux;
    };
    for (size_t t = 0; t < N; ++t) {
        if (t < full || sp == 1) {
            put(t, all[t], SYRK_NONE);
            continue;
        }
        const uint32_t first = (uint32_t)((t - full) * sp);
        w[2 * tl + 2 * (t - full)] = all[t];
        w[2 * tl + 2 * (t - full) + 1] = first << 8 | (uint32_t)sp;
        for (int k = 0; k < sp; ++k) put(full + first + k, all[t], (first + k) << 12 | (uint32_t)k << 6 | (uint32_t)sp);
    }
    // rendezvous counters of the persistent launch (zeroed by the upload), then the block address lists of the
    // problems whose X arrives in separate blocks, behind the tile table
    // (more than one round per XCD; measured in r02, L2-miss reads of a 14336-wide launch 37.5 against 49.6 GB with one tile
    // per workgroup, rocprofv3 FETCH_SIZE, +0.8 % speed: the switch to the one-tile form for every shape removed)
    if (kind == 2 && per_xcd > SYRK_GROUP) {
        pl.bar_word = (int64_t)w.size();
        w.insert(w.end(), SYRK_BAR_WORDS, 0u);
        // checkpoints: only when every problem of the launch walks the same number of half-stages (a dense block's inputs do;
        // MoE experts with their own token counts do not)
        const int64_t ck = o.ck;
        bool same = (ck & (ck - 1)) == 0 && ck >= 16;
        for (int k = 1; k < m && same; ++k) same = pl.p[k].Tp == pl.p[0].Tp;
        if (same && pl.p[0].Tp / 32 > ck) {
            pl.ck = (int)ck;
            pl.nck = (int)((pl.p[0].Tp / 32 - 1) / ck);
        }
    }
    if (w.size() & 1) w.push_back(SYRK_NONE);  // block addresses are 8 bytes
    for (int k = 0; k < m && kind == 2; ++k) {
        if (s[k].nseg <= 1) continue;
        pl.p[k].seg_word = (int64_t)w.size();
        pl.p[k].hs_per_seg = (int)(s[k].T / s[k].nseg / 32);
        w.insert(w.end(), 2 * (size_t)s[k].nseg, 0u);
    }
    pl.tl = tl;
    pl.per_xcd = per_xcd;
    pl.sp = sp;
    pl.total = pl.table_off + w.size() * 4;
    if (sp > 1) {
        pl.aux_word = (int64_t)tl;
        pl.reduce_word = (int64_t)(2 * tl);
        pl.n_reduce = (int)R;
        pl.partial_off = (pl.total + 255) & ~(size_t)255;
        pl.partial_bytes = R * sp * SYRK_SLOT_BYTES;
        pl.total = pl.partial_off + pl.partial_bytes;
    }
    // one tile per workgroup, or (rendezvous block present) one workgroup per CU walking its XCD's list in rounds
    // (option syrk_wgs, read per call: fewer resident workgroups for a fold that runs NEXT TO a latency-bound chain --
    // the block schedule's postponed folds -- so that the chain's kernels always find free CUs)
    int wgs = SYRK_CUS;
    if (const int64_t e = o.wgs) wgs = (e >= 8 && e <= SYRK_CUS) ? (int)(e & ~7) : SYRK_CUS;
    pl.grid = (unsigned)(pl.bar_word != SYRK_NO_WORD ? wgs : SYRK_XCDS * per_xcd);
    return pl;
}

}  // namespace gq
