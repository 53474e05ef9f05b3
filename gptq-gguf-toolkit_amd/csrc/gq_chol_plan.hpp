// gq_chol_plan.hpp -- the pure plan of one gq_h_prepare call's Cholesky chain (K2 + K3, gq_cholesky.hip; DESIGN.md K2+K3):
// the recursion flattened to steps in issue order, the regime of every node, the image-GEMM schedules with their place in
// the uploaded words, the layout of the workspace, and the bound that gq_workspace_bytes reports for it -- and the same for
// the stand-alone gq_chol_gemm.  Host arithmetic only, no HIP header: h_prepare, h_prepare_workspace_bytes, chol_gemm and
// tests/chol_plan_dump.cpp all read this one text.
#pragma once

#include <cstddef>
#include <cstdint>
#include <tuple>
#include <vector>

#include "gq_gemm3p_plan.hpp"

namespace gq {

constexpr int CHOL_NB = 128;         // leaf of the recursion, and the granularity of C
constexpr int P3_MAX_SLOTS = 1024;   // 256 MiB of K-split partial sums
constexpr size_t CHOL_PARTIAL_BYTES = (size_t)P3_MAX_SLOTS * p3::TILE * p3::TILE * 4;
constexpr int GEMM32_TK = 32;        // k per stage of gemm32_kernel (gq_gemm32.hpp: TK)
constexpr size_t CHOL_NO_REGION = ~(size_t)0;  // "this call has no such region"

// The options the chain reads, taken ONCE per entry-point call (chol_options, gq_cholesky.hip): a gq_option_set from
// another thread cannot give one call the workspace layout of one setting and the launches of another.
struct CholOptions {
    int64_t p3_min, b3_min;  // chol_3p_min (0: never), chol_3b_min
    int planes;              // chol_planes: 2 (row-scaled fp16 x 2, equilibrated matrix) or 3
    bool fp32, no_pair, no_equil, poison, diag_ref;  // chol_fp32, chol_no_pair, chol_no_equil, chol_poison, diag_ref
    int64_t gemm32_64_max;   // gemm32_64_max, for the paired launch only (launch_gemm32 chooses its own tile)
    auto key() const { return std::tie(p3_min, b3_min, planes, fp32, no_pair, no_equil, poison, diag_ref, gemm32_64_max); }
    bool operator<(const CholOptions& o) const { return key() < o.key(); }
};

// does launch_gemm32 (gq_gemm32.hpp) pick whole 64-tiles for a Cholesky-node product of this size?
inline bool gemm32_uses_64_full(int64_t M, int64_t N, int64_t K, bool lower, int64_t max64) {
    const int64_t tiles128 = ((M + 127) / 128) * ((N + 127) / 128) / (lower ? 2 : 1);
    return tiles128 < max64 && M % 64 == 0 && N % 64 == 0 && K % GEMM32_TK == 0;
}

// A node (n1 | n2) can run on pre-split operand images (gq_gemm3p.hpp) when both halves are multiples of 256 and at least
// p3_min wide ...
inline bool chol_p3_node(int64_t n1, int64_t n2, const CholOptions& o) {
    return o.p3_min > 0 && n1 >= o.p3_min && n2 >= o.p3_min && n1 % 256 == 0 && n2 % 256 == 0;
}
// ... and does so when the TOP node can: only then does the call carve images out of its workspace.
inline bool chol_uses_images(int64_t C, const CholOptions& o) {
    const int64_t nblk = C / CHOL_NB, mid = nblk / 2;
    return nblk >= 2 && chol_p3_node(mid * CHOL_NB, (nblk - mid) * CHOL_NB, o);
}

// Where the level-3 work of a node runs.
enum CholRegime {
    CHOL_IMAGE = 0,       // image GEMMs (gq_gemm3p.hpp); L21 X11 shares the SYRK update's launch, in front of the recursion into A22
    CHOL_SPLIT_BF16 = 1,  // fp32-accurate products on the bf16 matrix cores, split on the fly (gq_gemm3b.hpp): both halves >= b3_min
    CHOL_FP32 = 2,        // the fp32 instruction (gq_gemm32.hpp): small nodes are latency-bound
    CHOL_FP32_PAIR = 3,   // fp32, SYRK update and L21 X11 (both need only L21) as ONE launch of whole 64-tiles, in front of the
                          // recursion into A22 (bit-identical to separate launches: every output element is the same k-ordered chain)
};
struct CholNode {  // blocks [lo, mid) | [mid, hi) of CHOL_NB
    int64_t lo, mid, hi;
    CholRegime regime;
    int gemm[3];  // CHOL_IMAGE: its schedules in CholPlan::gemms -- L21 = A21 X11^T; SYRK update with L21 X11; X21 -- else -1
};
struct CholStep {
    enum Kind { LEAF = 0, NODE_FRONT = 1, NODE_BACK = 2 } kind;  // a node's launches in front of / behind the recursion into A22
    int at;                                                      // LEAF: the block; else the index into CholPlan::nodes
};
struct CholGemm {  // one image-GEMM launch: its schedule's place in the uploaded words
    size_t table_at, rlist_at;  // word offsets
    int n_reduce;
    std::vector<p3::GemmShape> shapes;  // what the schedule was made for (one problem, or two sharing the launch)
};
// Byte offsets from the 256-aligned workspace pointer.  The four image regions exist when the plan has image nodes, rmax
// and inv_scale only with 2 planes; the scales are reserved whether or not the call equilibrates.
struct CholLayout {
    size_t A, X;            // the reversed matrix / its factor's inverse, C x C fp32 each
    size_t dead, zc;        // C flags each
    size_t scales;          // C equilibration scales
    size_t img[2], partial; // two operand images of (C/2) x (C/2) x planes 16-bit values, the K-split partial sums
    size_t rmax, inv_scale; // [2][C/2] row maxima (bits) of the transposed operands, [2][C/2] epilogue scales
    size_t words;           // the upload
    size_t total;
};
struct CholPlan {
    int64_t C;
    int planes;
    bool images;                  // the call carves images and uploads words
    std::vector<CholStep> steps;  // in issue order
    std::vector<CholNode> nodes;
    std::vector<CholGemm> gemms;
    std::vector<uint32_t> words;  // the schedules of all image GEMMs, each starting on a multiple of 4 words
    bool too_many_slots;          // a schedule needs more than P3_MAX_SLOTS partial slots: the call refuses
    CholLayout at;
};

inline void chol_plan_add_gemm(CholPlan& pl, std::vector<p3::GemmShape> shapes) {
    const p3::Plan p = p3::make_plan(shapes, pl.planes == 3 ? 2 : 4, P3_MAX_SLOTS);
    CholGemm g;
    while (pl.words.size() % 4) pl.words.push_back(0u);
    g.table_at = pl.words.size();
    pl.words.insert(pl.words.end(), p.table.begin(), p.table.end());
    g.rlist_at = pl.words.size();
    pl.words.insert(pl.words.end(), p.rlist.begin(), p.rlist.end());
    g.n_reduce = (int)(p.rlist.size() / 2);
    g.shapes = std::move(shapes);
    if (p.nslots < 0) pl.too_many_slots = true;
    pl.gemms.push_back(std::move(g));
}

// Recursive blocked Cholesky WITH inverse (gq_cholesky.hip states the algebra): factor and invert [lo, mid), the node's
// front launches, factor and invert [mid, hi), the node's back launches.
inline void chol_plan_steps(CholPlan& pl, const CholOptions& o, int64_t lo, int64_t hi) {
    if (hi - lo == 1) {
        pl.steps.push_back({CholStep::LEAF, (int)lo});
        return;
    }
    const int64_t mid = (lo + hi) / 2;
    const int64_t n1 = (mid - lo) * CHOL_NB, n2 = (hi - mid) * CHOL_NB;
    chol_plan_steps(pl, o, lo, mid);
    CholNode nd{lo, mid, hi, CHOL_FP32, {-1, -1, -1}};
    if (pl.images && chol_p3_node(n1, n2, o)) {
        const int t1 = (int)(n1 / 256), t2 = (int)(n2 / 256), k1 = (int)(n1 / 32);
        nd.regime = CHOL_IMAGE;
        nd.gemm[0] = (int)pl.gemms.size();
        chol_plan_add_gemm(pl, {{t2, t1, k1, 1, false}});                         // L21 = A21 X11^T
        nd.gemm[1] = (int)pl.gemms.size();
        chol_plan_add_gemm(pl, {{t2, t2, k1, 0, true}, {t2, t1, k1, 2, false}});  // A22 -= L21 L21^T  and  L21 X11, one launch
    } else {
        const int64_t min3b = o.fp32 ? (int64_t)1 << 40 : o.b3_min;
        const bool pair = !o.no_pair && pl.C % 4 == 0 && gemm32_uses_64_full(n2, n2, n1, true, o.gemm32_64_max) &&
                          gemm32_uses_64_full(n2, n1, n1, false, o.gemm32_64_max);
        if (n1 >= min3b && n2 >= min3b) nd.regime = CHOL_SPLIT_BF16;
        else if (pair) nd.regime = CHOL_FP32_PAIR;
    }
    const int ni = (int)pl.nodes.size();
    pl.nodes.push_back(nd);
    pl.steps.push_back({CholStep::NODE_FRONT, ni});
    chol_plan_steps(pl, o, mid, hi);
    if (nd.regime == CHOL_IMAGE) {
        pl.nodes[ni].gemm[2] = (int)pl.gemms.size();
        chol_plan_add_gemm(pl, {{(int)(n2 / 256), (int)(n1 / 256), (int)(n2 / 32), 3, false}});  // X21 = -X22 (L21 X11)
    }
    pl.steps.push_back({CholStep::NODE_BACK, ni});
}

// Everything about one gq_h_prepare call that follows from C and the options, by arithmetic alone.  (gq_h_prepare refuses
// C % CHOL_NB != 0; gq_workspace_bytes answers for any C: the steps then cover the whole blocks, the layout C as it is.)
inline CholPlan make_chol_plan(int64_t C, const CholOptions& o) {
    CholPlan pl{};
    pl.C = C;
    pl.planes = o.planes == 3 ? 3 : 2;
    pl.images = chol_uses_images(C, o);
    if (C >= CHOL_NB) chol_plan_steps(pl, o, 0, C / CHOL_NB);
    const auto up256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t n = (size_t)C;
    CholLayout& at = pl.at;
    at.A = 0;
    at.X = at.A + n * n * 4;
    at.dead = at.X + n * n * 4;
    at.zc = at.dead + n;
    at.scales = up256(at.zc + n);
    at.total = at.scales + n * 4;
    at.img[0] = at.img[1] = at.partial = at.rmax = at.inv_scale = at.words = CHOL_NO_REGION;
    if (!pl.images) return pl;
    const size_t image = up256((n / 2) * (n / 2) * 2 * (size_t)pl.planes);
    at.img[0] = up256(at.zc + n) + up256(n * 4);
    at.img[1] = at.img[0] + image;
    at.partial = at.img[1] + image;
    size_t p = at.partial + CHOL_PARTIAL_BYTES;
    if (pl.planes == 2) {
        at.rmax = p;
        at.inv_scale = p + n * 4;
    }
    at.words = up256(p + 2 * n * 4);  // (3 planes: the two arrays are skipped, not used)
    at.total = at.words + pl.words.size() * 4;
    return pl;
}

// What gq_workspace_bytes(GQ_WS_H_PREPARE, ..) reports.  An upper BOUND of 255 (rounding the caller's pointer up to 256) +
// CholLayout::total (tests/test_chol_plan_cpu.py checks that it dominates).  The terms, in the order of the layout:
inline size_t chol_workspace_bytes(const CholPlan& pl) {
    const size_t C = (size_t)pl.C;
    size_t bytes = 2 * C * C * 4  // A and X
                   + 2 * C        // dead, zc
                   + 4 * C        // the equilibration scales
                   + 1024;        // rounding: the base pointer and the scales' start
    if (pl.images)
        bytes += 2 * ((C / 2) * (C / 2) * 2 * (size_t)pl.planes + 256)  // the two images, each rounded up to 256
                 + CHOL_PARTIAL_BYTES                                    // the partial sums
                 + pl.words.size() * 4                                   // the upload
                 + 4 * C * 4   // rmax and inv_scale, 2 C words together, and as many again that nothing uses
                 + 2048;       // rounding: the images' start and the upload's
    return bytes;
}

// ---- gq_chol_gemm: one product of the chain through the image path, for tests and benchmarks ----
struct CholGemmPlan {
    std::vector<uint32_t> words;  // [table | reduce list]
    size_t rlist_at;              // word offset
    int n_reduce;
    bool too_many_slots;
    // byte offsets from the 256-aligned workspace pointer, every region rounded up to 256: images of A (M x K) and B (N x K),
    // partial sums, row maxima of A and B, epilogue scales of A and B, the upload
    size_t ia, ib, partial, rma, rmb, isa, isb, words_at, total;
};
inline CholGemmPlan make_chol_gemm_plan(int planes, int64_t M, int64_t N, int64_t K, int kr, bool lower) {
    CholGemmPlan pl{};
    const p3::Plan p = p3::make_plan({p3::GemmShape{(int)(M / 256), (int)(N / 256), (int)(K / 32), kr, lower}}, planes == 3 ? 2 : 4,
                                     P3_MAX_SLOTS);
    pl.too_many_slots = p.nslots < 0;
    pl.words = p.table;
    pl.rlist_at = pl.words.size();
    pl.words.insert(pl.words.end(), p.rlist.begin(), p.rlist.end());
    pl.n_reduce = (int)(p.rlist.size() / 2);
    size_t at = 0;
    const auto take = [&](size_t bytes) {
        const size_t q = at;
        at += (bytes + 255) & ~(size_t)255;
        return q;
    };
    pl.ia = take((size_t)planes * 2 * M * K);
    pl.ib = take((size_t)planes * 2 * N * K);
    pl.partial = take(CHOL_PARTIAL_BYTES);
    pl.rma = take((size_t)M * 4);
    pl.rmb = take((size_t)N * 4);
    pl.isa = take((size_t)M * 4);
    pl.isb = take((size_t)N * 4);
    pl.words_at = take(pl.words.size() * 4);
    pl.total = at;
    return pl;
}
// What gq_workspace_bytes(GQ_WS_CHOL_GEMM, M, N, K, 0) reports: a bound of 255 + CholGemmPlan::total for either number of
// planes, by arithmetic on the shape alone.  The terms, in the order of the layout:
inline size_t chol_gemm_workspace_bound(int64_t M, int64_t N, int64_t K) {
    const size_t img = (size_t)3 * 2 * (size_t)K;  // bytes per operand row at 3 planes
    return img * (size_t)M + img * (size_t)N   // the images of A and B
           + CHOL_PARTIAL_BYTES                // the partial sums
           + 2 * (size_t)(M + N) * 4           // row maxima and epilogue scales of both operands
           + ((size_t)(M / 256 + 1) * (size_t)(N / 256 + 1) * 6 * 4 + 64) * 4  // the upload: units (4 words) and reduce entries (2) of the tiles, cut ones more than once
           + 4096;                             // rounding: the base pointer and the eight regions
}

}  // namespace gq
