// gq_walk.hpp -- host interface of the column walk (K5/K6 orchestration, gq_gptq.hip):
// the call record every entry point fills, the pure plan that the walk, gptq_workspace_bytes and
// gptq_uses_helper_stream all read, and the entry points gq_api.hip calls.
#pragma once

#include "gq_common.hpp"
#include "../../include/gptq_gguf_levels.h"

namespace gq {

// gq_scale_search.hip.  panel: the 256-byte panel block of a call chain (gq_common.hpp), row_ends / nstack: row-stacked
// matrices, each with its own panel-wide `continue`.
int launch_scale_search(const float* x, int64_t rows, int64_t ld, int q_type, const gq_search_t* p,
                        uint16_t* d, int64_t d_stride, uint8_t* s, int64_t s_ld, uint16_t* dmin,
                        int64_t dmin_stride, uint8_t* m, int64_t m_ld, hipStream_t st, unsigned* panel = nullptr,
                        const int64_t* row_ends = nullptr, int nstack = 1);

// What one walk over the columns quantizes to.  The walk itself -- segments, near and far updates -- is the same for all.
enum class WalkKind {
    KQuant,    // one K-quant type; several row-stacked matrices that share U count as one
    ActOrder,  // act_order (gptq.py:208-216, 233-235, 272-276): W and U arrive permuted, d / s / dmin / m are INPUTS (the
               // static scales of the original column groups, gptq.py:184-196), qweight comes back in permuted positions
    Uniform,   // the uniform grids of EvoPress' FastOBQ (evopress/src/fast_obq.py:146-200): the grid of a group is found
               // from W as it is when the block holding the group's first column starts (fast_obq.py:168-171)
    Bands,     // row bands of different K-quant types: only the lazy scale search is per band, and the segment kernel
               // reads the band table
    Iq4,       // the non-linear grids IQ4_XS / IQ4_NL (include/gptq_gguf_iq4_gptq.h): the scales of a 256-column group are found
               // lazily like a K-quant's, by the encoder's scale search; the segment kernel gets step / istep per 32-column block
};

struct UniformSpec {
    int bits, group, sym;  // group == 0: one grid per row, from the original W (fast_obq.py:153-154)
    float *scale, *zero;   // [R, C / group]
};
struct Iq4Spec {
    const float* importance;  // nullptr or [C]
    uint8_t* ls;              // IQ4_XS: [R, C / 32] (d of the call record is [R, C / 256]); IQ4_NL: unused (d is [R, C / 32])
    float *step, *istep;      // [R, C / 32]
};
struct BandPlan;  // the checked band table of gq_gptq_quantize_bands (gq_gptq.hip, next to the kernel that reads it)

struct WalkCall {
    WalkKind kind = WalkKind::KQuant;
    float* W = nullptr;        // [R, C] fp32, becomes the dequantized matrix
    const float* U = nullptr;  // [C, C]
    int64_t R = 0, C = 0;
    int block_size = 0;
    uint8_t* qweight = nullptr;
    uint16_t *d = nullptr, *dmin = nullptr;  // K-quant scales: outputs (KQuant, Bands), inputs (ActOrder), unused (Uniform)
    uint8_t *s = nullptr, *m = nullptr;
    void* ws = nullptr;
    size_t ws_bytes = 0;
    hipStream_t st = nullptr;
    // KQuant; ActOrder reads q_type, Bands reads p
    int q_type = -1;
    bool static_groups = false;  // gptq.py:184-196: all scales from the original W, before the walk
    const gq_search_t* p = nullptr;
    const int64_t* row_ends = nullptr;  // row-stacked matrices (rows never mix: gptq.py:222-270); only the scale searches
    int nstack = 1;                     // need to know where one ends and the next begins (their panel-wide `continue`)
    int32_t* researches_out = nullptr;  // gq_gptq_quantize_slice: receives the panel-wide re-search count
    // ActOrder
    const int32_t* perm = nullptr;
    // Uniform
    UniformSpec uni = {};
    // Bands
    const BandPlan* bands = nullptr;
    // Iq4 (reads q_type, writes d)
    Iq4Spec iq4 = {};
};

// The options the walk reads, taken ONCE per call (walk_options): a gq_option_set from another thread in the middle of
// a call does not reach that call.
struct WalkOptions {
    int64_t la, no_lookahead, far_sync, far_async_max_rows, far_async_min_sb, far_wgs, near64_maxn;
    bool helper_enabled;  // far_helper_enable
};
WalkOptions walk_options();

// Everything about a walk that follows from its shape and the options, by arithmetic alone (no HIP call).
struct WalkPlan {
    int64_t B;       // columns per block (gptq.py:54)
    int la;          // blocks per look-ahead super-block
    bool lookahead;  // errors of a super-block side by side, one chained far update behind it
    bool pair_look;  // near updates per 256-column group (the even block updates its partner in the segment kernel)
    bool helper_ok;  // the shape and the options admit far updates on the helper stream
    int64_t ldE;     // row stride of the error buffer
    int far_wgs;     // resident workgroups of the helper's far GEMM
    int64_t near64_maxn;
    // workspace layout: byte offsets from the workspace pointer rounded up to 256
    size_t err_off[2];  // error buffer [R, ldE]; the second one only with the helper stream (it may still read the
                        // previous super-block's errors while the walk writes the next one's)
    size_t blk_off;     // block scratch [R, B], present iff needs_blk
    size_t panel_off;   // the panel block of the scale searches (256 bytes)
    size_t total;       // what gq_workspace_bytes reports: a function of R and B alone
    bool needs_blk;     // some block of B columns is walked in several segments and lives in the block scratch
};
WalkPlan walk_plan(int64_t R, int64_t C, int block_size, WalkKind kind, int uniform_group, const WalkOptions& o);

size_t gptq_workspace_bytes(int64_t R, int64_t C, int block_size);
// does gq_gptq_quantize(R, C, block_size) put its far updates on the library's helper stream?
int gptq_uses_helper_stream(int64_t R, int64_t C, int block_size);
int far_helper_enable(int on);

// perm != nullptr: gq_gptq_quantize_perm
int gptq_quantize(float* W, const float* U, int64_t R, int64_t C, int q_type, int block_size, int static_groups,
                  const gq_search_t* p, uint8_t* qweight, uint16_t* d, uint8_t* s, uint16_t* dmin, uint8_t* m,
                  void* ws, size_t ws_bytes, hipStream_t st, const int32_t* perm, const int64_t* row_ends = nullptr,
                  int nstack = 1, int32_t* researches_out = nullptr);
int gptq_quantize_bands(float* W, const float* U, int64_t R, int64_t C, const gq_band_t* bands_host, int n_bands,
                        int block_size, const gq_search_t* p, uint8_t* qweight, uint16_t* d, uint8_t* s, uint16_t* dmin,
                        uint8_t* m, void* ws, size_t ws_bytes, hipStream_t st);
int obq_quantize(float* W, const float* U, int64_t R, int64_t C, int bits, int group_size, int sym, int block_size,
                 uint8_t* qweight, float* scale, float* zero, void* ws, size_t ws_bytes, hipStream_t st);

// include/gptq_gguf_iq4_gptq.h
int gptq_quantize_iq4(float* W, const float* U, int64_t R, int64_t C, int q_type, int block_size, const float* importance,
                      uint8_t* qweight, uint16_t* d, uint8_t* ls, float* step, float* istep, void* ws, size_t ws_bytes,
                      hipStream_t st);
// iq4/gq_iq4_gptq.hip: the scale search of gptq_gguf_iq4_encode.h on W[:, a : a + 256] as it is now -> d, ls, step, istep
int launch_iq4_scale_step(const float* W, int64_t R, int64_t C, int64_t a, bool xs, const float* importance, uint16_t* d,
                          uint8_t* ls, float* step, float* istep, hipStream_t st);

}  // namespace gq
