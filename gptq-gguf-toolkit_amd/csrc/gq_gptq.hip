// gq_gptq.hip -- K5 (per-column quantize + in-block error feedback), K6 (blocked
// trailing update) and the per-Linear orchestration of GPTQ.step.
//
// Reference: gptq.py:145-276.  Rows of W are independent given U, so K5 gives one
// LANE to a row (a wave = 64 rows) and walks the columns of a block in program
// order; U is wave-uniform and arrives through the scalar cache.  K6 is the
// GEMM W[:, c2:] -= Err[R,B] @ U[c1:c2, c2:] on the fp32 matrix cores
// (v_mfma_f32_32x32x2_f32 == a k-ordered fmaf chain, which is what the reference's
// sgemm computes per element -- verified bit-for-bit in tests/golden G6).
#include <atomic>
#include <mutex>
#include "gq_common.hpp"
#include "gq_gemm32.hpp"
#include "gq_walk.hpp"
#include "../../include/gptq_gguf_iq4.h"
#include "iq4/gq_iq4_search.hpp"
#include <stdlib.h>

namespace gq {

// ---------------------------------------------------------------- K5 segment
// Processes columns [a, a+len) (len <= 128, a % 16 == 0, len % 16 == 0) of the
// current block for 64 rows per wave.
//   src   : working values of these columns (W itself when the block is a single
//           segment, else the block scratch), row stride ld_src, already offset to
//           column a
//   W     : receives the dequantized column (gptq.py:266), row stride C
//   Err   : receives err (gptq.py:268) at column (a - c1) + i, row stride ld_err
//   qparams d/dmin [R, C/256], s/m [R, C/G] already hold the super-group of `a`
constexpr int SEG = 128;
constexpr int SB = 16;  // register sub-block
constexpr int SEG_WAVES = 8;  // wave 0 walks the dependent chain, all waves share the rank-1 tile updates
constexpr int SEG_NT = SEG / SB;
// working copy, U's diagonal block, two error tiles, the reciprocal diagonal and the group parameters of every tile
constexpr int SEG_LDS_BYTES = (SEG * 64 + SEG * SEG + 2 * SB * 64) * 4 + SEG * 8 + SEG_NT * 64 * 16;

// Correctly rounded fp32 division through an fp64 reciprocal: fl32(fl64(n * fl64(1 / d))) == fl32(n / d) for all
// finite fp32 n, d != 0.  The exact quotient of two 24-bit significands is either representable or at least 2^-49
// (relative) away from every fp32 rounding boundary (a boundary has 25 significant bits, so n - m d is a non-zero
// multiple of the unit of a 49-bit product), while the two fp64 roundings move the product by at most 2^-52: the
// final rounding sees the same side of every boundary as the exact quotient does.  Three VALU ops in the dependent
// chain (cvt, mul_f64, cvt) instead of the 11-instruction v_div_scale / v_rcp / fma / v_div_fixup sequence -- the
// column loop performs two divisions per column and is bound by exactly that chain.
__device__ __forceinline__ float div_rcp64(float n, double rd) { return (float)((double)n * rd); }

// BANDS (gq_gptq_quantize_bands): the rows are bands of different K-quant types that share U.  A workgroup owns 64 rows
// and band boundaries are multiples of 64, so it lies in exactly one band: it looks its band up in this table (it travels
// in the kernel arguments: wave-uniform scalar loads, no staging copy) and takes the type constants and its s / m base
// from there instead of from the launch-uniform arguments.  Everything per row is the code of the <false> instantiation.
struct BandTable {
    int32_t n;
    int32_t end64[GQ_BANDS_MAX];   // row_end / 64, ascending
    uint32_t info[GQ_BANDS_MAX];   // group | is_signed << 8 | (uint8_t)qmin << 16 | qmax << 24
    int64_t sm_off[GQ_BANDS_MAX];  // first byte of the band's [rows, C / group] block in s and in m
};
template <bool BANDS> struct BandArg {};
template <> struct BandArg<true> { BandTable t; };

// UNI: the uniform grid of EvoPress' FastOBQ (evopress/src/quant_utils.py:23-29) instead of a K-quant:
//   q = clamp(round(w / max(scale, 1e-9) + zero), 0, maxq),  w_hat = scale * (q - zero)
// with scale / zero fp32 [R, C / G] (uscale / uzero; d, s, dmin, m unused).
//
// The body is gq_segment_body.inc, shared with gptq_segment_iq4_kernel below.
template <bool PERM, bool UNI = false, bool BANDS = false>
__global__ __launch_bounds__(SEG_WAVES * 64) void gptq_segment_kernel(
    float* W, int64_t C, const float* src, int64_t ld_src,  // may alias (single-segment blocks)
    const float* __restrict__ U, int64_t a, int len, int64_t R,
    const uint16_t* __restrict__ d, const uint8_t* __restrict__ s, const uint16_t* __restrict__ dmin,
    const uint8_t* __restrict__ m, int G, int is_signed, float qmin, float qmax,
    uint8_t* __restrict__ qweight, float* __restrict__ Err, int64_t ld_err, int64_t err_col0,
    const int32_t* __restrict__ perm, const float* __restrict__ uscale = nullptr,
    const float* __restrict__ uzero = nullptr,  // PERM (act_order, gptq.py:211-216): column j takes the parameters of
                                                // the group of its ORIGINAL column perm[j]
    const float* __restrict__ Unext = nullptr,  // != nullptr: U[a .. a+127][a+128 .. a+255]; epilogue below
    int npair = 1,    // 2 (r05; needs Unext, src == W + a): this launch ALSO walks the partner block a+128 .. a+255 once its
                      // epilogue has brought this block's errors there -- every workgroup owns its 64 rows in both blocks, so
                      // nothing but the workgroup's own stores has to be visible: one launch per 256-column group instead of two
    BandArg<BANDS> bands = {}) {
    constexpr bool IQ4 = false;
    constexpr iq4::BestReg iq4tab{};  // (named by the discarded IQ4 branch)
#include "gq_segment_body.inc"
}

// IQ4 (gq_gptq_quantize_iq4, include/gptq_gguf_iq4_gptq.h): the walk on the non-linear grid of IQ4_XS / IQ4_NL.  The per-block
// parameters come the way UNI's do (G == 32): uscale = step, what the decoder multiplies kv[code] by, uzero = istep, the
// encoder's own inverse; code = best(istep * w), w_hat = step * kv[code].  Both are found by the lazy scale step
// (iq4/gq_iq4_gptq.hip) before the 256-column group is walked, so the pair launch applies.
// (A template so that the branches of the other forms are discarded unparsed, as they are in gptq_segment_kernel.)
template <bool ON = true>
__global__ __launch_bounds__(SEG_WAVES * 64) void gptq_segment_iq4_kernel(
    float* W, int64_t C, const float* src, int64_t ld_src, const float* __restrict__ U, int64_t a, int len, int64_t R,
    const float* __restrict__ uscale, const float* __restrict__ uzero, uint8_t* __restrict__ qweight, float* __restrict__ Err,
    int64_t ld_err, int64_t err_col0, const float* __restrict__ Unext, int npair) {
    constexpr bool PERM = !ON, UNI = ON, BANDS = !ON, IQ4 = ON;
    // what the K-quant and act_order forms read: unused here (every use sits in a discarded branch)
    const uint16_t *d = nullptr, *dmin = nullptr;
    const uint8_t *s = nullptr, *m = nullptr;
    const int32_t* perm = nullptr;
    int G = 32, is_signed = 0;
    float qmin = 0.0f, qmax = 15.0f;
    BandArg<BANDS> bands;
    (void)d, (void)dmin, (void)s, (void)m, (void)perm, (void)qmin, (void)qmax, (void)bands;
    iq4::BestReg iq4tab;
    iq4tab.init();
#include "gq_segment_body.inc"
}

// evopress/src/quant_utils.py:57-106 Quantizer.find_params(x, weight=True), perchannel: one wave per row of the
// [R, G] panel at x (row stride ld): min / max over the group, the symmetric range, (-1, +1) for a constant row,
// scale = (max - min) / maxq, zero = round(-min / scale) or (maxq + 1) / 2.  G % 4 == 0, x 16-byte aligned.
__global__ __launch_bounds__(256) void uniform_params_kernel(const float* __restrict__ x, int64_t R, int64_t ld, int G,
                                                             float maxq, int sym, float* __restrict__ scale,
                                                             float* __restrict__ zero, int64_t ng) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const float* xr = x + row * ld;
    float mn = xr[0], mx = mn;
    for (int j = lane * 4; j < G; j += 256) {
        const float4 v = *reinterpret_cast<const float4*>(xr + j);
        mn = fminf(fminf(mn, v.x), fminf(v.y, fminf(v.z, v.w)));
        mx = fmaxf(fmaxf(mx, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if (lane) return;
    if (sym) {
        mx = fmaxf(fabsf(mn), mx);
        if (mn < 0.0f) mn = -mx;
    }
    if (mn == mx) {
        mn = -1.0f;
        mx = 1.0f;
    }
    const float sc = (mx - mn) / maxq;
    scale[row * ng] = sc;
    zero[row * ng] = sym ? (maxq + 1.0f) / 2.0f : rintf(-mn / sc);
}

// Block scratch maintenance for block_size > 128 (generic path, VALU):
//   Wblk[r, j] = Wblk[r, j] + (-Err[r, e0+i]) * U[a+i, cj0+j]   for i = 0..n_i-1, in order.
__global__ __launch_bounds__(256) void block_far_update_kernel(float* __restrict__ Wblk, int64_t ld_blk,
                                                               int64_t ncols, int64_t R,
                                                               const float* __restrict__ Err, int64_t ld_err,
                                                               int64_t e0, int n_i, const float* __restrict__ U,
                                                               int64_t C, int64_t a, int64_t cj0) {
    const int64_t total = R * ncols;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / ncols, j = t % ncols;
        float w = Wblk[r * ld_blk + j];
        const float* e = Err + r * ld_err + e0;
        for (int i = 0; i < n_i; ++i) w = w + (-e[i]) * U[(a + i) * C + cj0 + j];
        Wblk[r * ld_blk + j] = w;
    }
}

__global__ __launch_bounds__(256) void copy2d_kernel(float* __restrict__ dst, int64_t ld_dst,
                                                     const float* __restrict__ src, int64_t ld_src, int64_t R,
                                                     int64_t ncols) {
    const int64_t total = R * ncols;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / ncols, j = t % ncols;
        dst[r * ld_dst + j] = src[r * ld_src + j];
    }
}

// ------------------------------------------------------------- K6 trailing update
// W[:, c2:] -= Err[R,B] @ U[c1:c2, c2:]  (gptq.py:270) on the fp32 matrix cores: see
// gq_gemm32.hpp (MODE 0: k-ordered fma chain from 0, then one subtraction).
int launch_trailing_update(float* Cmat, int64_t ldc, const float* A, int64_t lda, const float* B, int64_t ldb,
                           int64_t M, int64_t N, int64_t K, hipStream_t st) {
    ProfScope ps(PT_TRAILING, st);
    return launch_gemm32<false, 0, false>(Cmat, ldc, A, lda, B, ldb, M, N, K, st);
}

// ------------------------------------------------------------- orchestration
// One walk over the columns of W for every entry point (gq_walk.hpp): the entry points fill a
// WalkCall, walk_plan turns shape and options into the schedule and the workspace layout, and column_walk runs the
// named steps below block after block.
constexpr int LA = 8;      // look-ahead depth of the trailing update: blocks of 128 columns per super-block
constexpr int LA_B = 128;  // only this block size takes the look-ahead path (the chain length is a template constant)

static std::atomic<int> g_far_enabled{1};
int far_helper_enable(int on) { return g_far_enabled.exchange(on ? 1 : 0); }

// options are read per call: tests and A/B runs flip them inside one process
WalkOptions walk_options() {
    return WalkOptions{opt(OPT_la), opt(OPT_no_lookahead), opt(OPT_far_sync), opt(OPT_far_async_max_rows),
                       opt(OPT_far_async_min_sb), opt(OPT_far_wgs), opt(OPT_near64_maxn), g_far_enabled.load() != 0};
}

WalkPlan walk_plan(int64_t R, int64_t C, int block_size, WalkKind kind, int uniform_group, const WalkOptions& o) {
    WalkPlan p{};
    const int64_t B = p.B = block_size <= 0 || block_size > C ? C : block_size;  // gptq.py:54
    // tuning knob; even only: a 256-column scale-search group must not straddle two super-blocks
    p.la = (o.la >= 2 && o.la <= LA && o.la % 2 == 0) ? (int)o.la : LA;
    const int ug = kind == WalkKind::Uniform && uniform_group > 0 ? uniform_group : 0;
    // Look-ahead (B == 128): the blocks of a super-block of `la` blocks write their errors side by side into one
    // [R, LA * 128] buffer.  After a block only the REST OF THE SUPER-BLOCK is updated; at the end of the super-block
    // everything beyond it is updated by ONE chained GEMM (CHAIN = 128): per element ((w - E_0 U_0) - E_1 U_1) - ..., the
    // same operations in the same order as gptq.py:270 applied block after block, with one read and one write of W
    // instead of `la`.  A uniform group must lie inside one super-block as well: its grid is found from columns that
    // every earlier block has already updated.
    p.lookahead = B == LA_B && !o.no_lookahead && (!ug || (p.la * B) % ug == 0);
    // Near updates at the granularity of the 256-column scale-search groups: an even block hands its errors to its
    // partner (the odd block of the group) in the segment kernel's epilogue; after the odd block ONE chained launch
    // (K = 256, chain 128) brings both blocks' errors to the rest of the super-block.  Per element the same subtractions
    // in the same order as after-every-block updates; 3 launches per super-block instead of 7.  One launch after every
    // block remains for uniform groups that do not divide 256.
    p.pair_look = p.lookahead && p.la % 2 == 0 && (!ug || 256 % ug == 0);
    p.ldE = p.lookahead ? (int64_t)LA * B : B;
    p.helper_ok = p.lookahead && o.helper_enabled && !o.far_sync && R % 128 == 0 && C % 128 == 0 &&
                  R <= o.far_async_max_rows && C >= o.far_async_min_sb * (int64_t)p.la * B;
    p.far_wgs = (int)o.far_wgs;
    p.near64_maxn = o.near64_maxn;
    // The layout depends on R and B alone, never on the kind or the options: a caller sizes the workspace once.
    const size_t blk = (size_t)R * (size_t)B * sizeof(float);   // one block of errors, or of working values
    const size_t err = blk * (B == LA_B ? 2 * (size_t)LA : 1);  // super-block error buffer [R, LA * B], twice
    // wider than a segment, or -- B not dividing 256 -- a block that straddles a 256-column super-group and is therefore
    // walked in two segments
    p.needs_blk = B > SEG || (B > 0 && 256 % B != 0);
    p.err_off[0] = 0;
    p.err_off[1] = B == LA_B ? blk * LA : 0;
    p.blk_off = err;
    p.panel_off = (err + (p.needs_blk ? blk : 0) + 255) & ~(size_t)255;
    p.total = err + (p.needs_blk ? blk : 0) + 256 + 256;  // rounding up the workspace pointer, then the panel block
    return p;
}

size_t gptq_workspace_bytes(int64_t R, int64_t C, int block_size) {
    return walk_plan(R, C, block_size, WalkKind::KQuant, 0, walk_options()).total;
}
int gptq_uses_helper_stream(int64_t R, int64_t C, int block_size) {
    return walk_plan(R, C, block_size, WalkKind::KQuant, 0, walk_options()).helper_ok;
}

// band k is rows [row_end[k-1], row_end[k]) and has its own K-quant type
struct BandPlan {
    BandTable tbl;
    int q_type[GQ_BANDS_MAX];
    int64_t row_end[GQ_BANDS_MAX];
};

// when the K-quant scales of a 256-column group are found
enum class ScaleSearch {
    None,     // never: they are inputs (ActOrder), or there are none (Uniform)
    UpFront,  // gptq.py:184-196: all from the ORIGINAL W, before the first block
    Lazy,     // gptq.py:240-245: from W as it is when the walk reaches the group
};

struct Walk {  // a checked call: the record, its plan and the pointers both imply
    const WalkCall& c;
    WalkPlan p;
    TypeInfo ti;
    ScaleSearch search;
    float *err[2], *Wblk;
    unsigned* panel;  // one device word block shared by all scale-search launches of this call (each leaves it at zero)
    int64_t ng, nsg;  // groups / 256-column super-groups per row
    int gps;          // groups per super-group
    bool helper;      // far updates go through the helper stream: the plan admits it and the lease was granted
};
struct Block {  // gptq.py:222
    int64_t c1, c2;  // columns
    int64_t sb, pos;  // super-block and slot in it (0 without look-ahead)
    int64_t S0, S1;   // columns of the super-block
    bool single;      // one segment: the block fits in LDS and stays inside one 256-column super-group; else it lives
                      // in the block scratch
    float* Err;       // [R, ldE]
};

// Every check of a call, in the order the error messages have always had, then the plan and the workspace carve-up.
static int walk_open(const WalkCall& c, Walk& w) {
    const bool uni = c.kind == WalkKind::Uniform, iq = c.kind == WalkKind::Iq4;
    w.ti = TypeInfo{};
    if (iq) {
        if (c.q_type != GQ_IQ4_NL && c.q_type != GQ_IQ4_XS)
            GQ_FAIL(GQ_E_BAD_TYPE, "gq_gptq_quantize_iq4: q_type %d is neither GQ_IQ4_NL (20) nor GQ_IQ4_XS (23)", c.q_type);
        w.ti.group = 32;
        w.ti.qmax = 15;
    } else if (uni) {
        w.ti.group = c.uni.group > 0 ? c.uni.group : (int)c.C;
        w.ti.qmax = (1 << c.uni.bits) - 1;
    } else if (c.kind == WalkKind::Bands) {
        w.ti.group = 16;  // unused: every band brings its own
        for (int k = 0; k < c.bands->tbl.n; ++k) {
            TypeInfo tk;
            type_info(c.bands->q_type[k], tk);
            w.ti.k_search |= tk.k_search;
        }
    } else if (!type_info(c.q_type, w.ti)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_gptq_quantize: unknown q_type %d", c.q_type);
    if (c.R <= 0 || c.C <= 0 || c.C % 256)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gptq_quantize: R=%ld C=%ld (C %% 256 != 0)", (long)c.R, (long)c.C);
    if (!c.W || !c.U || !c.qweight || (!uni && !iq && (!c.d || !c.s || !c.dmin || !c.m)) ||
        (iq && (!c.d || !c.iq4.step || !c.iq4.istep || (c.q_type == GQ_IQ4_XS && !c.iq4.ls))))
        GQ_FAIL(GQ_E_NULL, "gq_gptq_quantize: null pointer");
    if (iq && !aligned(c.iq4.importance, 16)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gptq_quantize_iq4: importance not 16-byte aligned");
    w.p = walk_plan(c.R, c.C, c.block_size, c.kind, c.uni.group, walk_options());
    if (w.p.B % SB) GQ_FAIL(GQ_E_UNSUPPORTED, "gq_gptq_quantize: block_size %ld is not a multiple of 16", (long)w.p.B);
    if (c.kind == WalkKind::ActOrder && c.q_type == GQ_Q3_K)
        GQ_FAIL(GQ_E_UNSUPPORTED, "gq_gptq_quantize_perm: Q3_K forces act_order off (gptq.py:204-206)");
    if (c.kind == WalkKind::Bands || iq) w.search = ScaleSearch::Lazy;
    else if (c.kind != WalkKind::KQuant) w.search = ScaleSearch::None;
    else w.search = c.static_groups && c.q_type != GQ_Q3_K ? ScaleSearch::UpFront : ScaleSearch::Lazy;  // gptq.py:204-206
    if (!c.ws || c.ws_bytes < w.p.total)
        GQ_FAIL(GQ_E_WORKSPACE, "gq_gptq_quantize: workspace %zu < %zu bytes", c.ws_bytes, w.p.total);
    char* base = reinterpret_cast<char*>(((uintptr_t)c.ws + 255) & ~(uintptr_t)255);
    w.err[0] = reinterpret_cast<float*>(base + w.p.err_off[0]);
    w.err[1] = reinterpret_cast<float*>(base + w.p.err_off[1]);
    w.Wblk = reinterpret_cast<float*>(base + w.p.blk_off);
    w.panel = reinterpret_cast<unsigned*>(base + w.p.panel_off);
    w.ng = c.C / w.ti.group;
    w.nsg = c.C / 256;
    w.gps = uni ? 1 : 256 / w.ti.group;
    w.helper = false;
    return GQ_OK;
}

// quant_utils.py:57-106 for the [R, G] panel at column `col`: grid g of every row
static void uniform_params(const Walk& w, int64_t col, int G, int64_t g) {
    const WalkCall& c = w.c;
    hipLaunchKernelGGL(uniform_params_kernel, dim3((unsigned)((c.R + 3) / 4)), dim3(256), 0, c.st, c.W + col, c.R, c.C, G,
                       (float)w.ti.qmax, c.uni.sym, c.uni.scale + g, c.uni.zero + g, w.ng);
}

// Uniform: fast_obq.py:168-171 for every group that starts inside this block
static int uniform_grids(const Walk& w, const Block& b) {
    const int64_t G = w.c.uni.group;
    ProfScope ps(PT_SCALE_SEARCH, w.c.st);
    for (int64_t g = (b.c1 + G - 1) / G; g * G < b.c2; ++g) uniform_params(w, g * G, (int)G, g);
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

// gptq.py:184-196: all scales from the ORIGINAL W
static int up_front_search(const Walk& w) {
    const WalkCall& c = w.c;
    int rc;
    for (int64_t col = 0; col < c.C; col += 256)
        if ((rc = launch_scale_search(c.W + col, c.R, c.C, c.q_type, c.p, c.d + col / 256, w.nsg, c.s + (col / 256) * w.gps,
                                      w.ng, c.dmin + col / 256, w.nsg, c.m + (col / 256) * w.gps, w.ng, c.st, w.panel,
                                      c.row_ends, c.nstack)))
            return rc;
    return GQ_OK;
}

// gptq.py:240-245 for the 256-column group that starts at column a.  Reads w (global), NOT w_blk: with block_size > 256
// these columns are stale by design.  Bands: one launch per band, on that band's rows.
static int lazy_search(const Walk& w, int64_t a) {
    const WalkCall& c = w.c;
    const int64_t sg = a / 256, nsg = w.nsg;
    if (c.kind == WalkKind::Iq4)
        return launch_iq4_scale_step(c.W, c.R, c.C, a, c.q_type == GQ_IQ4_XS, c.iq4.importance, c.d, c.iq4.ls, c.iq4.step,
                                     c.iq4.istep, c.st);
    if (c.kind != WalkKind::Bands)
        return launch_scale_search(c.W + a, c.R, c.C, c.q_type, c.p, c.d + sg, nsg, c.s + sg * w.gps, w.ng, c.dmin + sg, nsg,
                                   c.m + sg * w.gps, w.ng, c.st, w.panel, c.row_ends, c.nstack);
    const BandPlan& bp = *c.bands;
    int rc;
    for (int k = 0; k < bp.tbl.n; ++k) {
        const int64_t r0 = k ? bp.row_end[k - 1] : 0, rows = bp.row_end[k] - r0;
        const int gk = (int)(bp.tbl.info[k] & 0xffu), gpsk = 256 / gk;
        const int64_t ngk = c.C / gk;
        uint8_t *sk = c.s + bp.tbl.sm_off[k] + sg * gpsk, *mk = c.m + bp.tbl.sm_off[k] + sg * gpsk;
        if ((rc = launch_scale_search(c.W + r0 * c.C + a, rows, c.C, bp.q_type[k], c.p, c.d + r0 * nsg + sg, nsg, sk, ngk,
                                      c.dmin + r0 * nsg + sg, nsg, mk, ngk, c.st, w.panel)))
            return rc;
    }
    return GQ_OK;
}

static int segment_attributes() {
    static std::atomic<bool> seg_attr{false};  // guards an idempotent call: a race sets the same value twice
    if (seg_attr) return GQ_OK;
    for (const void* k : {(const void*)gptq_segment_kernel<false>, (const void*)gptq_segment_kernel<true>,
                          (const void*)gptq_segment_kernel<false, true>, (const void*)gptq_segment_kernel<false, false, true>,
                          (const void*)gptq_segment_iq4_kernel<>})
        GQ_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, SEG_LDS_BYTES));
    seg_attr = true;
    return GQ_OK;
}

// K5 for columns [a, a + len) of block b: the one place that picks the kernel instantiation of a kind.
// unext != nullptr: the partner's columns are updated in the epilogue; npair == 2: and walked in the same launch.
static int launch_segment(const Walk& w, const Block& b, int64_t a, int len, const float* unext, int npair) {
    const WalkCall& c = w.c;
    const TypeInfo& ti = w.ti;
    const dim3 grid((unsigned)((c.R + 63) / 64)), block(SEG_WAVES * 64);
    const float* src = b.single ? c.W + a : w.Wblk + (a - b.c1);
    const int64_t ld_src = b.single ? c.C : w.p.B, ldE = w.p.ldE, err_col0 = b.pos * w.p.B + (a - b.c1);
    ProfScope ps(PT_GPTQ_SEGMENT, c.st);
    switch (c.kind) {
    case WalkKind::Bands:
        hipLaunchKernelGGL((gptq_segment_kernel<false, false, true>), grid, block, SEG_LDS_BYTES, c.st, c.W, c.C, src, ld_src,
                           c.U, a, len, c.R, c.d, c.s, c.dmin, c.m, 0, 0, 0.0f, 0.0f, c.qweight, b.Err, ldE, err_col0, nullptr,
                           nullptr, nullptr, unext, npair, BandArg<true>{c.bands->tbl});
        break;
    case WalkKind::Uniform:  // d, s, dmin, m are null: the UNI instantiation never reads them
        hipLaunchKernelGGL((gptq_segment_kernel<false, true>), grid, block, SEG_LDS_BYTES, c.st, c.W, c.C, src, ld_src, c.U, a,
                           len, c.R, c.d, c.s, c.dmin, c.m, ti.group, 0, 0.0f, (float)ti.qmax, c.qweight, b.Err, ldE, err_col0,
                           nullptr, c.uni.scale, c.uni.zero, unext);
        break;
    case WalkKind::Iq4:
        hipLaunchKernelGGL(gptq_segment_iq4_kernel<>, grid, block, SEG_LDS_BYTES, c.st, c.W, c.C, src, ld_src, c.U, a, len, c.R,
                           (const float*)c.iq4.step, (const float*)c.iq4.istep, c.qweight, b.Err, ldE, err_col0, unext, npair);
        break;
    case WalkKind::ActOrder:
        hipLaunchKernelGGL(gptq_segment_kernel<true>, grid, block, SEG_LDS_BYTES, c.st, c.W, c.C, src, ld_src, c.U, a, len, c.R,
                           c.d, c.s, c.dmin, c.m, ti.group, ti.is_signed, (float)ti.qmin, (float)ti.qmax, c.qweight, b.Err, ldE,
                           err_col0, c.perm, nullptr, nullptr, unext, npair);
        break;
    case WalkKind::KQuant:
        hipLaunchKernelGGL(gptq_segment_kernel<false>, grid, block, SEG_LDS_BYTES, c.st, c.W, c.C, src, ld_src, c.U, a, len, c.R,
                           c.d, c.s, c.dmin, c.m, ti.group, ti.is_signed, (float)ti.qmin, (float)ti.qmax, c.qweight, b.Err, ldE,
                           err_col0, nullptr, nullptr, nullptr, unext, npair);
        break;
    }
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

// The columns of block b, segment after segment.  walked_by_partner: in, this block's columns were already walked by the
// previous (even) block's launch; out, this block's last launch walked the next block as well.
static int walk_block(const Walk& w, const Block& b, bool& walked_by_partner) {
    const WalkCall& c = w.c;
    const int64_t B = w.p.B;
    int rc;
    if (!b.single) {  // w_blk lives in scratch
        ProfScope ps(PT_BLOCK_FAR, c.st);
        hipLaunchKernelGGL(copy2d_kernel, dim3(2048), dim3(256), 0, c.st, w.Wblk, B, c.W + b.c1, c.C, c.R, b.c2 - b.c1);
        GQ_LAUNCH_CHECK();
    }
    int64_t a = walked_by_partner ? b.c2 : b.c1;
    walked_by_partner = false;
    while (a < b.c2) {
        // a segment never crosses a 256-column super-group boundary: the lazy
        // scale search (gptq.py:240-245) must see W as it is at that column.
        int64_t e = a + SEG < b.c2 ? a + SEG : b.c2;
        const int64_t next_sg = (a / 256 + 1) * 256;
        if (e > next_sg) e = next_sg;
        const int len = (int)(e - a);
        if (w.search == ScaleSearch::Lazy && (a % 256) == 0 && (rc = lazy_search(w, a))) return rc;
        // an even block of a 256-group: its partner's columns are updated in this kernel's epilogue
        const float* unext =
            (w.p.pair_look && b.single && len == SEG && !(b.pos & 1) && b.c2 + B <= c.C) ? c.U + a * c.C + a + SEG : nullptr;
        // the partner block in the same launch (it is a whole single segment too: B == SEG, c2 + B <= C)
        const int npair = (unext && c.kind != WalkKind::Uniform && B == SEG) ? 2 : 1;
        walked_by_partner = npair == 2;
        if ((rc = launch_segment(w, b, a, len, unext, npair))) return rc;
        if (e < b.c2) {  // push this segment's rank-1 updates into the rest of the block
            ProfScope ps(PT_BLOCK_FAR, c.st);
            hipLaunchKernelGGL(block_far_update_kernel, dim3(2048), dim3(256), 0, c.st, w.Wblk + (e - b.c1), B, b.c2 - e, c.R,
                               b.Err, w.p.ldE, a - b.c1, len, c.U, c.C, a, e);
            GQ_LAUNCH_CHECK();
        }
        a = e;
    }
    return GQ_OK;
}

// ---- after a block: gptq.py:270, W[:, c2:] -= Err @ U[c1:c2, c2:], cut four ways ----

// this block's errors to the columns [c2, end): every later column without look-ahead, else the rest of the super-block
static int block_trailing_update(const Walk& w, const Block& b, int64_t end) {
    const WalkCall& c = w.c;
    return launch_trailing_update(c.W + b.c2, c.C, b.Err + b.pos * w.p.B, w.p.ldE, c.U + b.c1 * c.C + b.c2, c.C, c.R,
                                  end - b.c2, b.c2 - b.c1, c.st);
}

// pair_look, after the odd block of a 256-group: both blocks' errors, in order, to the rest of the super-block (the even
// block reached its partner in the segment kernel).  What was measured against this form: DESIGN.md K6.
static int pair_near_update(const Walk& w, const Block& b) {
    if (!(b.pos & 1)) return GQ_OK;
    const WalkCall& c = w.c;
    const int64_t B = w.p.B, n = b.S1 - b.c2;
    const float *E = b.Err + (b.pos - 1) * B, *Up = c.U + (b.c1 - B) * c.C + b.c2;
    ProfScope ps(PT_TRAILING, c.st);
    // up to near64_maxn columns: 64x64 tiles with the K = 256 panels whole in LDS (gemm32_near256_kernel)
    if (n <= w.p.near64_maxn && c.R % 64 == 0) return launch_gemm32_near256(c.W + b.c2, c.C, E, w.p.ldE, Up, c.C, c.R, n, c.st);
    return launch_gemm32<false, 0, false, 0, LA_B>(c.W + b.c2, c.C, E, w.p.ldE, Up, c.C, c.R, n, 2 * B, c.st);
}

// end of a super-block, caller's stream only: all its blocks at once, every later column
static int far_update(const Walk& w, const Block& b) {
    const WalkCall& c = w.c;
    ProfScope ps(PT_TRAILING_FAR, c.st);
    return launch_gemm32<false, 0, false, 0, LA_B>(c.W + b.S1, c.C, b.Err, w.p.ldE, c.U + b.S0 * c.C + b.S1, c.C, c.R,
                                                   c.C - b.S1, b.S1 - b.S0, c.st);
}

// ---- the far update next to the walk (single-Linear look-ahead pipeline) ----
// One helper stream per device, held by ONE call at a time: from the start of its enqueue until its last helper launch
// has finished on the device.  A call that finds it taken runs the one-stream schedule (same results) -- several
// chains funnelled through one in-order helper stream would wait for each other's GEMMs (measured: 103 -> 112 ms
// per block step with all seven Linears on it).
struct FarHelper {
    hipStream_t st = nullptr;
    hipEvent_t done = nullptr;  // recorded behind the holder's last helper launch
    bool enqueueing = false, recorded = false;
};
static std::mutex g_far_mu;
static FarHelper g_far[64];
static int far_helper_acquire(FarHelper** out) {
    *out = nullptr;
    int dev = 0;
    GQ_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_far_mu);
    FarHelper& h = g_far[dev & 63];
    if (!h.st) {  // a plain stream with persistent launches; a CU-masked one was measured and dropped
        GQ_HIP(hipStreamCreateWithFlags(&h.st, hipStreamNonBlocking));
        GQ_HIP(hipEventCreateWithFlags(&h.done, hipEventDisableTiming));
    }
    if (h.enqueueing) return GQ_OK;
    if (h.recorded && hipEventQuery(h.done) != hipSuccess) {
        (void)hipGetLastError();  // hipErrorNotReady is not an error
        return GQ_OK;
    }
    h.enqueueing = true;
    *out = &h;
    return GQ_OK;
}
static void far_helper_release(FarHelper* h) {
    if (!h) return;
    std::lock_guard<std::mutex> lk(g_far_mu);
    h->recorded = hipEventRecord(h->done, h->st) == hipSuccess;
    h->enqueueing = false;
}
struct FarHold {  // releases on every return path of the walk
    FarHelper* h = nullptr;
    ~FarHold() { far_helper_release(h); }
};
// re-recordable events of the calling host thread (a wait captures the record that precedes it)
static int far_event(int i, hipEvent_t* out) {
    thread_local hipEvent_t pool[96] = {};
    hipEvent_t& e = pool[i % 96];
    if (!e) GQ_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    *out = e;
    return GQ_OK;
}

// The far update of super-block s (everything beyond it) is one MFMA-bound GEMM; the walk of super-block s+1 is a string
// of small latency-bound launches that needs the far update on ITS OWN G = la * 128 columns only.  So the far update is
// cut by column groups (g = index of a group of G columns; F_s[g] = super-block s's update of group g):
//   caller's stream:  walk(s) | F_s[s+1] | walk(s+1)            | F_{s+1}[s+2] | walk(s+2) ...
//   helper stream:                       | F_s[s+2] , F_s[s+3..] |              | F_{s+1}[s+3] , F_{s+1}[s+4..] ...
// The helper's launches of super-block s are released BEHIND F_s[s+1] (the event `ready`), not next to it: the walk
// waits for F_s[s+1], so that launch gets every CU; the helper stream is in order, so while it is still busy with
// F_{s-1}[..] the later release costs it nothing, and once it is idle it has the whole walk(s+1) to catch up.
// F_s[s+1] waits for F_{s-1}[s+1] (an event after that small launch); the helper launches are PERSISTENT with a
// bounded number of workgroups, so the walk's kernels always find free CUs instead of queueing behind 56-us GEMM
// tiles.  Every element of W still sees ((w - E_0 U_0) - E_1 U_1) - ... in the same order: results are unchanged.
// The error buffer is doubled (the helper may still read super-block s's errors while the walk fills s+1's).
struct FarPipeline {
    FarHold hold;
    hipStream_t helper = nullptr;
    hipEvent_t ev_small_prev = nullptr;         // behind F_{s-1}[s+1]
    hipEvent_t ev_bulk[2] = {nullptr, nullptr}; // behind the helper's last read of each half of the error buffer
    hipEvent_t ev_last = nullptr;               // behind the helper's last launch
    int ev_i = 0;                               // events taken from far_event so far

    // helper stays null when another call holds the stream: that call runs the one-stream schedule
    int lease() {
        int rc;
        if ((rc = far_helper_acquire(&hold.h))) return rc;
        if (hold.h) helper = hold.h->st;
        return GQ_OK;
    }
    // before super-block sb writes its half of the error buffer: the helper is done with it
    int wait_for_half(hipStream_t st, int64_t sb) {
        if (!ev_bulk[sb & 1]) return GQ_OK;
        GQ_HIP(hipStreamWaitEvent(st, ev_bulk[sb & 1], 0));
        ev_bulk[sb & 1] = nullptr;
        return GQ_OK;
    }
    // end of super-block b.sb: F_s[s+1] on the caller's stream, F_s[s+2] and F_s[s+3..] on the helper
    int far_update(const Walk& w, const Block& b) {
        const WalkCall& c = w.c;
        const int64_t C = c.C, S0 = b.S0, S1 = b.S1, ldE = w.p.ldE, K = S1 - S0;
        const int64_t G = (int64_t)w.p.la * w.p.B, g1 = S1 + G < C ? S1 + G : C, g2 = g1 + G < C ? g1 + G : C;
        const float* Us = c.U + S0 * C;
        hipEvent_t ready = nullptr, ev = nullptr;
        int rc;
        if (ev_small_prev) GQ_HIP(hipStreamWaitEvent(c.st, ev_small_prev, 0));  // F_{s-1}[s+1] is in
        ev_small_prev = nullptr;
        {
            ProfScope ps(PT_TRAILING_FAR, c.st);
            if ((rc = launch_gemm32_chain_full<LA_B>(c.W + S1, C, b.Err, ldE, Us + S1, C, c.R, g1 - S1, K, c.st))) return rc;
        }
        if (g1 >= C) return GQ_OK;
        // the helper's two launches of this super-block queue behind F_s[s+1]: the walk waits for that one, so it
        // gets the whole chip instead of the CUs the helper's persistent workgroups leave over
        if ((rc = far_event(ev_i++, &ready))) return rc;
        GQ_HIP(hipEventRecord(ready, c.st));
        GQ_HIP(hipStreamWaitEvent(helper, ready, 0));
        ProfScope ps(PT_TRAILING_FAR, helper);
        if ((rc = launch_gemm32_chain_full<LA_B>(c.W + g1, C, b.Err, ldE, Us + g1, C, c.R, g2 - g1, K, helper, w.p.far_wgs)))
            return rc;
        if ((rc = far_event(ev_i++, &ev))) return rc;
        GQ_HIP(hipEventRecord(ev, helper));
        ev_small_prev = ev;
        if (g2 < C &&
            (rc = launch_gemm32_chain_full<LA_B>(c.W + g2, C, b.Err, ldE, Us + g2, C, c.R, C - g2, K, helper, w.p.far_wgs)))
            return rc;
        if ((rc = far_event(ev_i++, &ev))) return rc;
        GQ_HIP(hipEventRecord(ev, helper));
        ev_bulk[b.sb & 1] = ev;
        ev_last = ev;
        return GQ_OK;
    }
    // the caller's stream sees the helper's last write
    int final_wait(hipStream_t st) {
        if (ev_last) GQ_HIP(hipStreamWaitEvent(st, ev_last, 0));
        return GQ_OK;
    }
};

static int column_walk(const WalkCall& c) {
    Walk w{c};
    int rc;
    if ((rc = walk_open(c, w))) return rc;
    const WalkPlan& p = w.p;
    FarPipeline far;
    if (p.helper_ok) {
        if ((rc = far.lease())) return rc;
        w.helper = far.helper != nullptr;
    }
    if ((w.ti.k_search && w.search != ScaleSearch::None) || c.researches_out) GQ_HIP(hipMemsetAsync(w.panel, 0, 256, c.st));
    if (c.kind == WalkKind::Uniform && c.uni.group <= 0) {
        uniform_params(w, 0, (int)c.C, 0);
        GQ_LAUNCH_CHECK();
    }
    if (w.search == ScaleSearch::UpFront && (rc = up_front_search(w))) return rc;
    if ((rc = segment_attributes())) return rc;

    bool walked_by_partner = false;
    for (int64_t c1 = 0; c1 < c.C; c1 += p.B) {  // gptq.py:222
        Block b;
        b.c1 = c1;
        b.c2 = c1 + p.B < c.C ? c1 + p.B : c.C;
        b.single = (b.c2 - b.c1) <= SEG && (b.c1 / 256 == (b.c2 - 1) / 256);
        const int64_t bi = c1 / p.B;
        b.sb = bi / p.la;
        b.pos = p.lookahead ? bi % p.la : 0;
        b.S0 = b.sb * p.la * p.B;
        b.S1 = b.S0 + p.la * p.B < c.C ? b.S0 + p.la * p.B : c.C;
        b.Err = w.err[w.helper ? b.sb & 1 : 0];
        if (w.helper && b.pos == 0 && (rc = far.wait_for_half(c.st, b.sb))) return rc;
        if (c.kind == WalkKind::Uniform && c.uni.group > 0 && (rc = uniform_grids(w, b))) return rc;
        if ((rc = walk_block(w, b, walked_by_partner))) return rc;
        if (b.c2 >= c.C) break;
        if (!p.lookahead) rc = block_trailing_update(w, b, c.C);
        else if (b.c2 < b.S1) rc = p.pair_look ? pair_near_update(w, b) : block_trailing_update(w, b, b.S1);
        else rc = w.helper ? far.far_update(w, b) : far_update(w, b);
        if (rc) return rc;
    }
    if ((rc = far.final_wait(c.st))) return rc;
    if (c.researches_out)  // every scale search of this call ran on `st`: the count is final here
        GQ_HIP(hipMemcpyAsync(c.researches_out, w.panel + GQ_PANEL_RESEARCH, sizeof(int32_t), hipMemcpyDeviceToDevice, c.st));
    return GQ_OK;
}

static WalkCall walk_call(WalkKind kind, float* W, const float* U, int64_t R, int64_t C, int block_size, uint8_t* qweight,
                          void* ws, size_t ws_bytes, hipStream_t st) {
    WalkCall c;
    c.kind = kind;
    c.W = W, c.U = U, c.R = R, c.C = C, c.block_size = block_size;
    c.qweight = qweight;
    c.ws = ws, c.ws_bytes = ws_bytes, c.st = st;
    return c;
}

int gptq_quantize(float* W, const float* U, int64_t R, int64_t C, int q_type, int block_size, int static_groups,
                  const gq_search_t* p, uint8_t* qweight, uint16_t* d, uint8_t* s, uint16_t* dmin, uint8_t* m,
                  void* ws, size_t ws_bytes, hipStream_t st, const int32_t* perm, const int64_t* row_ends, int nstack,
                  int32_t* researches_out) {
    if (nstack > 1 && perm) GQ_FAIL(GQ_E_UNSUPPORTED, "gq_gptq_quantize_stacked: act_order matrices are not stacked");
    WalkCall c = walk_call(perm ? WalkKind::ActOrder : WalkKind::KQuant, W, U, R, C, block_size, qweight, ws, ws_bytes, st);
    c.d = d, c.s = s, c.dmin = dmin, c.m = m;
    c.q_type = q_type;
    c.static_groups = static_groups != 0;
    c.p = p;
    c.row_ends = row_ends, c.nstack = nstack, c.researches_out = researches_out;
    c.perm = perm;
    return column_walk(c);
}

// gq_gptq_quantize_iq4 (include/gptq_gguf_iq4_gptq.h); walk_open makes every check
int gptq_quantize_iq4(float* W, const float* U, int64_t R, int64_t C, int q_type, int block_size, const float* importance,
                      uint8_t* qweight, uint16_t* d, uint8_t* ls, float* step, float* istep, void* ws, size_t ws_bytes,
                      hipStream_t st) {
    WalkCall c = walk_call(WalkKind::Iq4, W, U, R, C, block_size, qweight, ws, ws_bytes, st);
    c.q_type = q_type;
    c.d = d;
    c.iq4 = Iq4Spec{importance, ls, step, istep};
    return column_walk(c);
}

// gq_gptq_quantize_bands (include/gptq_gguf_levels.h): every check of the band table before the first HIP call.
int gptq_quantize_bands(float* W, const float* U, int64_t R, int64_t C, const gq_band_t* bands_host, int n_bands,
                        int block_size, const gq_search_t* p, uint8_t* qweight, uint16_t* d, uint8_t* s, uint16_t* dmin,
                        uint8_t* m, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!bands_host) GQ_FAIL(GQ_E_NULL, "gq_gptq_quantize_bands: null band table");
    if (n_bands < 1 || n_bands > GQ_BANDS_MAX)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gptq_quantize_bands: %d bands (1..%d)", n_bands, GQ_BANDS_MAX);
    if (R <= 0 || C <= 0 || C % 256) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gptq_quantize_bands: R=%ld C=%ld (C %% 256 != 0)", (long)R, (long)C);
    BandPlan bp{};
    bp.tbl.n = n_bands;
    int64_t prev = 0, off = 0;
    for (int k = 0; k < n_bands; ++k) {
        const int64_t e = bands_host[k].row_end;
        TypeInfo tk;
        if (!type_info(bands_host[k].q_type, tk))
            GQ_FAIL(GQ_E_BAD_TYPE, "gq_gptq_quantize_bands: band %d has unknown q_type %d", k, (int)bands_host[k].q_type);
        if (e % 64 || e <= prev || e > R || e / 64 > INT32_MAX)
            GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gptq_quantize_bands: band %d ends at row %ld (ascending multiples of 64 up to R=%ld)", k,
                    (long)e, (long)R);
        bp.q_type[k] = bands_host[k].q_type;
        bp.row_end[k] = e;
        bp.tbl.end64[k] = (int32_t)(e / 64);
        bp.tbl.info[k] = (uint32_t)tk.group | (uint32_t)tk.is_signed << 8 | (uint32_t)(uint8_t)(int8_t)tk.qmin << 16 |
                         (uint32_t)tk.qmax << 24;
        bp.tbl.sm_off[k] = off;
        off += (e - prev) * (C / tk.group);
        prev = e;
    }
    if (prev != R) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_gptq_quantize_bands: the last band ends at row %ld, R=%ld", (long)prev, (long)R);
    WalkCall c = walk_call(WalkKind::Bands, W, U, R, C, block_size, qweight, ws, ws_bytes, st);
    c.d = d, c.s = s, c.dmin = dmin, c.m = m;
    c.p = p;
    c.bands = &bp;
    return column_walk(c);
}

// EvoPress FastOBQ.step for one bit width (evopress/src/fast_obq.py:146-200) given U.
int obq_quantize(float* W, const float* U, int64_t R, int64_t C, int bits, int group_size, int sym, int block_size,
                 uint8_t* qweight, float* scale, float* zero, void* ws, size_t ws_bytes, hipStream_t st) {
    if (bits < 1 || bits > 8) GQ_FAIL(GQ_E_UNSUPPORTED, "gq_obq_quantize: bits=%d (1..8: qweight is uint8)", bits);
    if (!scale || !zero) GQ_FAIL(GQ_E_NULL, "gq_obq_quantize: null pointer");
    if (group_size < 0 || (group_size > 0 && (group_size % SB || C % group_size)))
        GQ_FAIL(GQ_E_UNSUPPORTED, "gq_obq_quantize: group_size %d must be 0 or a multiple of 16 that divides C=%ld", group_size, (long)C);
    WalkCall c = walk_call(WalkKind::Uniform, W, U, R, C, block_size, qweight, ws, ws_bytes, st);
    c.uni = UniformSpec{bits, group_size, sym ? 1 : 0, scale, zero};
    return column_walk(c);
}

}  // namespace gq
