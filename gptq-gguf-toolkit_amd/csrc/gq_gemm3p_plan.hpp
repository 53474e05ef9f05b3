// gq_gemm3p_plan.hpp -- the host-side schedule of one image-GEMM launch (gq_gemm3p.hpp, which includes this file and
// describes the scheduling in its header comment).  Host arithmetic only, no HIP header: gq_gemm3p.hpp's kernels read the
// table it builds, gq_chol_plan.hpp lays the tables of a whole factorisation out, tests/chol_plan_dump.cpp prints them.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace gq {
namespace p3 {

constexpr int BLK = 8192;                 // one image block: [128 rows][32 k] 16-bit
constexpr int TILE = 256;
constexpr int CPT = 8;                    // chunks per 256 k
constexpr int T_UNITS = 260, NWG = 256;

// ------------------------------------------------------------------------------------------------ host: schedule
// kr: k-range of a tile in IMAGE chunks, always [0, len):  0: KC;  1: 8 (tn + 1)  (B^T lower-triangular);
// 2: KC - 8 tn (B lower-triangular, imaged in reverse);  3: 8 (tm + 1) (A lower-triangular).  lower: tm >= tn only.
struct GemmShape {
    int MT, NT, KC, kr;
    bool lower;
};
struct Plan {
    std::vector<uint32_t> table;    // what the kernel reads (counters, queue bounds, units)
    std::vector<uint32_t> rlist;    // reduce list (2 words per split tile)
    int nslots = 0;
    double makespan = 0, ideal = 0;  // in chunks per workgroup (diagnostics)
};
inline int tile_len(const GemmShape& s, int tm, int tn) {
    int len = s.KC;
    if (s.kr == 1) len = std::min(s.KC, CPT * (tn + 1));
    else if (s.kr == 2) len = s.KC - CPT * tn;
    else if (s.kr == 3) len = std::min(s.KC, CPT * (tm + 1));
    return len;
}
// Schedule.  Tiles in super-tile order (8 x 4 blocks sharing 12 operand panels, longest blocks first) form ONE sequence;
// it is cut into 8 contiguous segments of equal work, one per XCD (a cut may fall inside a tile: K-split).  Inside an
// XCD the 32 workgroups take the segment's units round-robin -- so the 32 units running at a time are neighbours in
// the sequence -- for as many whole rounds as stay below the XCD's mean load T; what is left is dealt by the
// wrap-around rule (fill workgroup after workgroup up to T, cutting a tile along k where it overflows): every
// workgroup ends within a few chunks of T, with at most ~33 cut tiles per XCD.  Unit lengths are multiples of `gran`
// chunks (NP = 3: 2, NP = 2: 4; every k boundary is a multiple of 128 = 4 chunks); the cost of a unit is its length plus
// OVH chunks (prologue + epilogue).
inline Plan make_plan(const std::vector<GemmShape>& shapes, int gran, int max_slots) {
    constexpr int OVH = 2, MINP = 8;
    const int slot_base = 0;
    struct Tile { int prob, tm, tn, len; };
    std::vector<Tile> tiles;
    struct Blk { int neg_len, prob, bi, bj; };
    std::vector<Blk> blocks;
    for (int prob = 0; prob < (int)shapes.size(); ++prob) {
        const GemmShape& s = shapes[prob];
        const bool by_m = s.kr == 3;
        const int bm = by_m ? 4 : 8, bn = by_m ? 8 : 4;
        const int nbm = (s.MT + bm - 1) / bm, nbn = (s.NT + bn - 1) / bn;
        for (int bi = 0; bi < nbm; ++bi)
            for (int bj = 0; bj < nbn; ++bj) {
                int mx = 0;
                for (int tm = bi * bm; tm < std::min(s.MT, (bi + 1) * bm); ++tm)
                    for (int tn = bj * bn; tn < std::min(s.NT, (bj + 1) * bn); ++tn)
                        if (!s.lower || tm >= tn) mx = std::max(mx, tile_len(s, tm, tn));
                if (mx > 0) blocks.push_back({-mx, prob, bi, bj});
            }
    }
    std::stable_sort(blocks.begin(), blocks.end(), [](const Blk& a, const Blk& b) { return a.neg_len < b.neg_len; });
    for (auto& b : blocks) {
        const GemmShape& s = shapes[b.prob];
        const bool by_m = s.kr == 3;
        const int bm = by_m ? 4 : 8, bn = by_m ? 8 : 4;
        for (int tm = b.bi * bm; tm < std::min(s.MT, (b.bi + 1) * bm); ++tm)
            for (int tn = b.bj * bn; tn < std::min(s.NT, (b.bj + 1) * bn); ++tn)
                if (!s.lower || tm >= tn) {
                    const int len = tile_len(s, tm, tn);
                    if (len > 0) tiles.push_back({b.prob, tm, tn, len});
                }
    }
    struct Piece { int tile, cb, ce; };
    long total = 0;
    for (auto& t : tiles) total += t.len + OVH;
    // 1. XCD segments
    std::vector<Piece> seg[8];
    {
        long acc = 0;
        int x = 0;
        for (int ti = 0; ti < (int)tiles.size(); ++ti) {
            int at = 0;
            const int len = tiles[ti].len;
            while (at < len) {
                const long end_x = (x == 7) ? (long)1 << 60 : (total * (x + 1)) / 8;
                long room = end_x - acc - OVH;  // chunks of this tile the segment still takes
                int take = len - at;
                if (room < take) {
                    int r = (int)std::max<long>(room, 0) / gran * gran;
                    if (r < MINP) r = 0;                      // too short a head: the whole rest goes to the next XCD
                    if (take - r < MINP) r = take;            // too short a tail: keep it here
                    take = r;
                }
                if (take > 0) {
                    seg[x].push_back({ti, at, at + take});
                    acc += take + OVH;
                    at += take;
                }
                if (at < len || acc >= end_x) {
                    if (x < 7) ++x;
                    else if (take == 0) { seg[x].push_back({ti, at, len}); acc += len - at + OVH; at = len; }
                }
            }
        }
    }
    // 2. per XCD: whole rounds, then wrap-around; T grows from the mean load until everything fits
    std::vector<Piece> wg[NWG];
    double mk = 0;
    for (int x = 0; x < 8; ++x) {
        long tot = 0;
        for (auto& p : seg[x]) tot += p.ce - p.cb + OVH;
        std::vector<Piece> mine[32];
        long load[32];
        for (long T = (tot + 31) / 32;; T += gran) {
            for (int w = 0; w < 32; ++w) { load[w] = 0; mine[w].clear(); }
            size_t done = 0;
            while (done + 32 <= seg[x].size()) {
                bool ok = true;
                for (int w = 0; w < 32 && ok; ++w) {
                    const Piece& p = seg[x][done + w];
                    ok = load[w] + (p.ce - p.cb) + OVH <= T;
                }
                if (!ok) break;
                for (int w = 0; w < 32; ++w) {
                    const Piece& p = seg[x][done + w];
                    load[w] += p.ce - p.cb + OVH;
                    mine[w].push_back(p);
                }
                done += 32;
            }
            int w = 0;
            bool fits = true;
            for (size_t i = done; i < seg[x].size() && fits; ++i) {
                Piece p = seg[x][i];
                while (p.cb < p.ce) {
                    if (w > 31) { fits = false; break; }
                    const int len = p.ce - p.cb;
                    const long room = T - load[w] - OVH;
                    int take;
                    if (room >= len) take = len;
                    else {
                        take = (int)(std::max<long>(room, 0) / gran * gran);
                        if (len - take < MINP) take = (len - MINP) / gran * gran;  // never leave a stub
                        if (take < MINP) { ++w; continue; }                        // nor start with one
                    }
                    mine[w].push_back({p.tile, p.cb, p.cb + take});
                    load[w] += take + OVH;
                    p.cb += take;
                }
            }
            if (fits) break;
        }
        for (int w = 0; w < 32; ++w) {
            wg[w * 8 + x] = mine[w];
            mk = std::max(mk, (double)load[w]);
        }
    }
    // 3. slots for the tiles that ended up in more than one piece (pieces of a tile in k order), the table
    std::vector<int> npieces(tiles.size(), 0), first_slot(tiles.size(), -1), seen(tiles.size(), 0);
    for (int b = 0; b < NWG; ++b)
        for (auto& p : wg[b]) ++npieces[p.tile];
    Plan pl;
    int slots = 0;
    for (size_t t = 0; t < tiles.size(); ++t)
        if (npieces[t] > 1) {
            first_slot[t] = slot_base + slots;
            slots += npieces[t];
            pl.rlist.push_back((uint32_t)tiles[t].prob << 28 | (uint32_t)tiles[t].tm << 14 | (uint32_t)tiles[t].tn);
            pl.rlist.push_back((uint32_t)first_slot[t] << 8 | (uint32_t)npieces[t]);
        }
    pl.nslots = slots;
    pl.table.assign(T_UNITS, 0u);
    unsigned at = 0;
    for (int b = 0; b < NWG; ++b) {
        pl.table[b] = at;
        for (auto& p : wg[b]) {
            const Tile& t = tiles[p.tile];
            pl.table.push_back((uint32_t)t.prob << 28 | (uint32_t)t.tm << 14 | (uint32_t)t.tn);
            pl.table.push_back((uint32_t)p.cb);
            pl.table.push_back((uint32_t)p.ce);
            pl.table.push_back(npieces[p.tile] > 1 ? (uint32_t)(first_slot[p.tile] + seen[p.tile]++ + 1) : 0u);
            ++at;
        }
    }
    pl.table[NWG] = at;
    pl.makespan = mk;
    pl.ideal = (double)total / NWG;
    if (slots > max_slots) pl.nslots = -1;  // the caller refuses (never at the sizes of this path: <= ~35 cut tiles per XCD)
    return pl;
}

}  // namespace p3
}  // namespace gq
