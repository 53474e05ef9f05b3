// gq_switch.hip -- K18: one candidate of the bit-width search made current.  gq_level_switch takes a HOST table of jobs
// (stored level -> live weight, packed K-quant blocks or a dense matrix as the source) and applies up to
// GQ_SWITCH_MAX_JOBS of them per launch; the reference's load_layers (evopress/evo_quant_search.py:110-138) reads a dense
// file from disk per changed Linear instead.
//
// The table travels in the kernel arguments (SwitchTable, 3080 bytes of the 4 KB segment): no staging buffer, no copy on
// the stream, nothing to keep alive after the call returns.  Entry j carries the prefix sum `unit_end` of work units of
// jobs 0 .. j; workgroup u (one unit each) finds its job by a binary search over that column -- all of it on block-uniform
// values, i.e. scalar loads from the argument segment and scalar compares -- and then runs ONE turn of the job's kind:
//   packed: blockdec::decode_turn<QT, OutT>, the very function gq_dequantize_blocks' kernel loops over (16 blocks of 256
//           values staged in LDS with the type's natural load width, 16 values per thread, 16-byte stores).  Same text,
//           same flags, so the same bits; reads and writes stay inside the job's own [src, ..) and [dst, ..) as there.
//   dense : 512 chunks of 16 output bytes, two per thread, chunk k = (row k / cpr, 16 / elsize columns): one 8- / 16- /
//           32-byte load of the (gathered) source row, exact widening to fp32, one RNE cast (f2h / f2bf: torch's
//           .to(dtype)), one 16-byte store.
//   Q8_0  : blockdec::decode_turn_b32<QT, OutT>, gq_dequantize_blocks' turn for that type: 128 blocks of 32 values -- the same
//           4096 values per unit --, 2-byte staging loads, half a block per thread.
//   IQ4_XS takes the packed arm (a 256-value type with 8-byte staging loads), IQ4_NL Q8_0's (include/gptq_gguf_iq4.h).
// The kind / out_dtype dispatch is a switch on block-uniform values: a workgroup executes one arm.  HBM-bound like K15:
// 0.33-0.82 B/param in, 2 or 4 B/param out; the unit is K15's turn so that the per-byte rate is K15's.
// The three unit functions live in gq_switch_units.hpp, shared with gq_switch_experts.hip (K30: a job of E stacked matrices).
#include "../../../include/gptq_gguf_iq4.h"  // (includes gptq_gguf_q8.h and gptq_gguf_search.h)
#include "gq_block_host.hpp"
#include "gq_switch_units.hpp"

namespace gq {
namespace {

using namespace blockdec;
using namespace switchunit;  // the units themselves: gq_switch_units.hpp, shared with gq_switch_experts.hip

struct SwitchEntry {
    const uint8_t* src;
    uint8_t* dst;
    const int32_t* row_src;
    int64_t n;          // packed: blocks of the job (R * C / 256; Q8_0 / IQ4_NL: R * C / 32); dense: 16-byte output chunks (R * cpr)
    int32_t per_row;    // packed: blocks per row; dense: chunks per row (cpr)
    uint32_t unit_end;  // work units of entries 0 .. this one
    int32_t kind, out_dtype;
};
struct SwitchTable {
    int32_t n;
    int32_t pad;
    SwitchEntry e[GQ_SWITCH_MAX_JOBS];
};
static_assert(sizeof(SwitchTable) <= 4096 - 64, "the job table must fit the kernel-argument segment");

__global__ __launch_bounds__(256) void level_switch_kernel(const SwitchTable t) {
    __shared__ __attribute__((aligned(16))) uint8_t sb[SB_BYTES];
    __shared__ int64_t ssrc[SSRC_N];
    const uint32_t u = blockIdx.x;
    int lo = 0, hi = t.n - 1;  // the first entry whose unit_end exceeds u (the grid is e[n - 1].unit_end: it exists)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (u < t.e[mid].unit_end) hi = mid;
        else lo = mid + 1;
    }
    const SwitchEntry& J = t.e[lo];
    const int64_t ul = (int64_t)(u - (lo ? t.e[lo - 1].unit_end : 0u));  // the unit within the job
    switch (J.kind) {
    case GQ_Q2_K: packed_unit<GQ_Q2_K>(J, ul * DB, sb, ssrc); break;
    case GQ_Q3_K: packed_unit<GQ_Q3_K>(J, ul * DB, sb, ssrc); break;
    case GQ_Q4_K: packed_unit<GQ_Q4_K>(J, ul * DB, sb, ssrc); break;
    case GQ_Q5_K: packed_unit<GQ_Q5_K>(J, ul * DB, sb, ssrc); break;
    case GQ_Q6_K: packed_unit<GQ_Q6_K>(J, ul * DB, sb, ssrc); break;
    case GQ_IQ4_XS: packed_unit<GQ_IQ4_XS>(J, ul * DB, sb, ssrc); break;
    case GQ_Q8_0: b32_unit<GQ_Q8_0>(J, ul * B32_DB, sb, ssrc); break;
    case GQ_IQ4_NL: b32_unit<GQ_IQ4_NL>(J, ul * B32_DB, sb, ssrc); break;
    case GQ_F32: dense_unit_from<GQ_F32>(J, ul * DENSE_CHUNKS); break;
    case GQ_F16: dense_unit_from<GQ_F16>(J, ul * DENSE_CHUNKS); break;
    default: dense_unit_from<GQ_BF16>(J, ul * DENSE_CHUNKS); break;
    }
}

bool is_dtype(int d) { return d == GQ_F32 || d == GQ_F16 || d == GQ_BF16; }
int elsize(int d) { return d == GQ_F32 ? 4 : 2; }

constexpr int64_t MAX_UNITS = 0x7fffffff;  // of one launch (the grid's x extent) and so of one job

// every check of job i; fills the job's table entry except unit_end, and its unit count
int check_job(const gq_switch_job_t& j, int i, SwitchEntry& e, int64_t& units) {
    const int bs = block_geometry(j.kind).bs;  // values per block; 0: not a packed type
    if (!bs && !is_dtype(j.kind)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_level_switch: job %d: unknown kind %d", i, j.kind);
    if (!is_dtype(j.out_dtype)) GQ_FAIL(GQ_E_BAD_TYPE, "gq_level_switch: job %d: unknown out_dtype %d", i, j.out_dtype);
    if (!j.src) GQ_FAIL(GQ_E_NULL, "gq_level_switch: job %d: src is NULL", i);
    if (!j.dst) GQ_FAIL(GQ_E_NULL, "gq_level_switch: job %d: dst is NULL", i);
    if (j.R < 1) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_level_switch: job %d: R=%ld (R < 1)", i, (long)j.R);
    if (j.C < 1 || j.C > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_level_switch: job %d: C=%ld (not in [1, 2^31))", i, (long)j.C);
    if (!aligned(j.dst, 16)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_level_switch: job %d: dst not 16-byte aligned", i);
    if (!aligned(j.row_src, 4)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_level_switch: job %d: row_src not 4-byte aligned", i);
    const int des = elsize(j.out_dtype);
    int64_t per_unit;
    if (bs) {
        if (j.C % bs) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_level_switch: job %d: C=%ld (C %% %d != 0)", i, (long)j.C, bs);
        if (!aligned(j.src, block_align(j.kind)))
            GQ_FAIL(GQ_E_BAD_SHAPE, "gq_level_switch: job %d: src not %d-byte aligned", i, block_align(j.kind));
        e.per_row = (int32_t)(j.C / bs), per_unit = bs == 32 ? B32_DB : DB;
    } else {
        const int ses = elsize(j.kind);
        if (j.C * ses % 16 || j.C * des % 16)
            GQ_FAIL(GQ_E_BAD_SHAPE, "gq_level_switch: job %d: C=%ld (rows of src and dst must be multiples of 16 bytes)", i, (long)j.C);
        if (!aligned(j.src, 16)) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_level_switch: job %d: src not 16-byte aligned", i);
        e.per_row = (int32_t)(j.C * des / 16), per_unit = DENSE_CHUNKS;
    }
    if (j.R > (MAX_UNITS * per_unit) / e.per_row)
        GQ_FAIL(GQ_E_BAD_SHAPE, "gq_level_switch: job %d: R=%ld C=%ld is more than one launch takes", i, (long)j.R, (long)j.C);
    e.src = static_cast<const uint8_t*>(j.src), e.dst = static_cast<uint8_t*>(j.dst), e.row_src = j.row_src;
    e.n = j.R * e.per_row, e.kind = j.kind, e.out_dtype = j.out_dtype;
    units = (e.n + per_unit - 1) / per_unit;
    return GQ_OK;
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_level_switch(const gq_switch_job_t* jobs_host, int n_jobs, void* stream) {
    if (int rc = options_ok()) return rc;
    if (n_jobs < 0) GQ_FAIL(GQ_E_BAD_SHAPE, "gq_level_switch: n_jobs=%d (n_jobs < 0)", n_jobs);
    if (n_jobs == 0) return GQ_OK;
    if (!jobs_host) GQ_FAIL(GQ_E_NULL, "gq_level_switch: jobs_host is NULL");
    SwitchEntry e;
    int64_t units;
    for (int i = 0; i < n_jobs; ++i)  // all refusals first: a refused call has launched nothing
        if (int rc = check_job(jobs_host[i], i, e, units)) return rc;
    hipStream_t st = (hipStream_t)stream;
    SwitchTable t;
    for (int i = 0; i < n_jobs;) {
        int64_t total = 0;
        t.n = 0, t.pad = 0;
        while (i < n_jobs && t.n < GQ_SWITCH_MAX_JOBS) {
            check_job(jobs_host[i], i, t.e[t.n], units);
            if (total + units > MAX_UNITS) break;  // (a single job never exceeds it: checked above)
            total += units;
            t.e[t.n++].unit_end = (uint32_t)total;
            ++i;
        }
        for (int k = t.n; k < GQ_SWITCH_MAX_JOBS; ++k) t.e[k] = SwitchEntry{};
        hipLaunchKernelGGL(level_switch_kernel, dim3((unsigned)total), dim3(256), 0, st, t);
        GQ_LAUNCH_CHECK();
    }
    return GQ_OK;
}

}  // extern "C"
