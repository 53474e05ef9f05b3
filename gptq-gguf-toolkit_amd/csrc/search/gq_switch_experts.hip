// gq_switch_experts.hip -- K30: the level switch of a stacked expert tensor.  gq_level_switch_experts takes a HOST table of
// jobs, each one GGUF tensor `blk.N.ffn_{gate,up,down}_exps.weight` ([E, R, C], packed blocks or dense) and the E destination
// matrices it belongs in (expert e at dst + e * dst_expert_stride: the gate or up half of transformers' gate_up_proj
// [E, 2I, H], or down_proj), and applies up to GQ_SWITCH_EXPERTS_MAX_JOBS of them per launch.
//
// The table travels in the kernel arguments as gq_level_switch's does (ExpertsTable, 3984 bytes of the 4 KB segment).  Entry j
// carries the prefix sum `unit_end` of the work units of jobs 0 .. j and the units of ONE expert, `upe`: a work unit never
// straddles experts.  Workgroup u finds its job by the binary search of search/gq_switch.hip over `unit_end`, its expert and
// its unit within the expert by one 32-bit division -- all on block-uniform values, i.e. scalar loads from the argument segment
// and scalar arithmetic -- and then runs ONE unit of gq_switch_units.hpp on that expert's [R, C] matrix: the text
// gq_level_switch runs for the job (src + e * slice, dst + e * stride, NULL, R, C, kind, out_dtype), so the same bits, the same
// reads inside the expert's slice and the same writes inside the expert's destination matrix.
#include "../../../include/gptq_gguf_moe_search.h"
#include "gq_block_host.hpp"
#include "gq_switch_units.hpp"

namespace gq {
namespace {

using namespace blockdec;
using namespace switchunit;

struct ExpertsEntry {
    const uint8_t* src;
    uint8_t* dst;
    int64_t n;           // of ONE expert: packed: blocks; dense: 16-byte output chunks (SwitchEntry's n for the [R, C] matrix)
    int64_t src_stride;  // bytes from an expert's slice of src to the next
    int64_t dst_stride;  // bytes from an expert's destination matrix to the next
    int32_t per_row;     // packed: blocks per row; dense: chunks per row
    uint32_t upe;        // work units of one expert
    uint32_t unit_end;   // work units of entries 0 .. this one (E * upe each)
    int16_t kind, out_dtype;
};
struct ExpertsTable {
    int32_t n;
    int32_t pad;
    ExpertsEntry e[GQ_SWITCH_EXPERTS_MAX_JOBS];
};
constexpr size_t TABLE_ROOM = 4096 - 64;  // what gq_level_switch's table is held to
static_assert(sizeof(ExpertsTable) <= TABLE_ROOM, "the job table must fit the kernel-argument segment");
static_assert(sizeof(ExpertsTable) + sizeof(ExpertsEntry) > TABLE_ROOM, "GQ_SWITCH_EXPERTS_MAX_JOBS is the largest count that fits");

// one expert's matrix as the units of gq_switch_units.hpp take a job
struct ExpertJob {
    const uint8_t* src;
    uint8_t* dst;
    const int32_t* row_src;  // always NULL: expert tensors carry no rotary permutation
    int64_t n;
    int32_t per_row;
    int32_t out_dtype;
};

__global__ __launch_bounds__(256) void level_switch_experts_kernel(const ExpertsTable t) {
    __shared__ __attribute__((aligned(16))) uint8_t sb[SB_BYTES];
    __shared__ int64_t ssrc[SSRC_N];
    const uint32_t u = blockIdx.x;
    int lo = 0, hi = t.n - 1;  // the first entry whose unit_end exceeds u (the grid is e[n - 1].unit_end: it exists)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (u < t.e[mid].unit_end) hi = mid;
        else lo = mid + 1;
    }
    const ExpertsEntry& J = t.e[lo];
    const uint32_t uj = u - (lo ? t.e[lo - 1].unit_end : 0u);  // the unit within the job
    const uint32_t ex = uj / J.upe, ul = uj - ex * J.upe;      // its expert (< E: unit_end counts E * upe), the unit within it
    const ExpertJob X = {J.src + (int64_t)ex * J.src_stride, J.dst + (int64_t)ex * J.dst_stride, nullptr, J.n, J.per_row, J.out_dtype};
    run_unit(X, J.kind, (int64_t)ul, sb, ssrc);
}

bool is_dtype(int d) { return d == GQ_F32 || d == GQ_F16 || d == GQ_BF16; }
int elsize(int d) { return d == GQ_F32 ? 4 : 2; }

constexpr int64_t MAX_UNITS = 0x7fffffff;  // of one launch (the grid's x extent) and so of one job
constexpr int64_t MAX_E = 65535;
#define WHO "gq_level_switch_experts"

// every check of job i; fills the job's table entry except unit_end, and its unit count
int check_job(const gq_switch_experts_job_t& j, int i, ExpertsEntry& e, int64_t& units) {
    const int bs = block_geometry(j.kind).bs, ts = block_geometry(j.kind).ts;  // values / bytes per block; 0: not a packed type
    if (!bs && !is_dtype(j.kind)) GQ_FAIL(GQ_E_BAD_TYPE, WHO ": job %d: unknown kind %d", i, j.kind);
    if (!is_dtype(j.out_dtype)) GQ_FAIL(GQ_E_BAD_TYPE, WHO ": job %d: unknown out_dtype %d", i, j.out_dtype);
    if (!j.src) GQ_FAIL(GQ_E_NULL, WHO ": job %d: src is NULL", i);
    if (!j.dst) GQ_FAIL(GQ_E_NULL, WHO ": job %d: dst is NULL", i);
    if (j.E < 1 || j.E > MAX_E) GQ_FAIL(GQ_E_BAD_SHAPE, WHO ": job %d: E=%ld (not in [1, %ld])", i, (long)j.E, (long)MAX_E);
    if (j.R < 1) GQ_FAIL(GQ_E_BAD_SHAPE, WHO ": job %d: R=%ld (R < 1)", i, (long)j.R);
    if (j.C < 1 || j.C > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, WHO ": job %d: C=%ld (not in [1, 2^31))", i, (long)j.C);
    if (!aligned(j.dst, 16)) GQ_FAIL(GQ_E_BAD_SHAPE, WHO ": job %d: dst not 16-byte aligned", i);
    const int des = elsize(j.out_dtype);
    int64_t per_unit, row_bytes;
    int al;
    if (bs) {
        if (j.C % bs) GQ_FAIL(GQ_E_BAD_SHAPE, WHO ": job %d: C=%ld (C %% %d != 0)", i, (long)j.C, bs);
        al = block_align(j.kind);
        e.per_row = (int32_t)(j.C / bs), per_unit = bs == 32 ? B32_DB : DB, row_bytes = (int64_t)e.per_row * ts;
    } else {
        const int ses = elsize(j.kind);
        if (j.C * ses % 16 || j.C * des % 16)
            GQ_FAIL(GQ_E_BAD_SHAPE, WHO ": job %d: C=%ld (rows of src and dst must be multiples of 16 bytes)", i, (long)j.C);
        al = 16;
        e.per_row = (int32_t)(j.C * des / 16), per_unit = DENSE_CHUNKS, row_bytes = j.C * ses;
    }
    if (!aligned(j.src, al)) GQ_FAIL(GQ_E_BAD_SHAPE, WHO ": job %d: src not %d-byte aligned", i, al);
    if (j.R > (MAX_UNITS * per_unit) / e.per_row)
        GQ_FAIL(GQ_E_BAD_SHAPE, WHO ": job %d: R=%ld C=%ld is more than one launch takes", i, (long)j.R, (long)j.C);
    e.n = j.R * e.per_row;
    const int64_t upe = (e.n + per_unit - 1) / per_unit;
    if (upe * j.E > MAX_UNITS)
        GQ_FAIL(GQ_E_BAD_SHAPE, WHO ": job %d: E=%ld R=%ld C=%ld is more than one launch takes", i, (long)j.E, (long)j.R, (long)j.C);
    e.src_stride = j.R * row_bytes;  // (R * row_bytes <= 2^31 * 2048 * 34: no overflow)
    if (j.E > 1 && e.src_stride % al)
        GQ_FAIL(GQ_E_BAD_SHAPE, WHO ": job %d: R=%ld C=%ld: an expert's slice of src (%ld bytes) breaks the type's %d-byte alignment",
                i, (long)j.R, (long)j.C, (long)e.src_stride, al);
    if (j.dst_expert_stride < j.R * j.C || j.dst_expert_stride > (int64_t)1 << 44)
        GQ_FAIL(GQ_E_BAD_SHAPE, WHO ": job %d: dst_expert_stride=%ld (not in [R * C = %ld, 2^44])", i, (long)j.dst_expert_stride,
                (long)(j.R * j.C));
    if (j.dst_expert_stride * des % 16)
        GQ_FAIL(GQ_E_BAD_SHAPE, WHO ": job %d: dst_expert_stride=%ld (not a multiple of 16 bytes)", i, (long)j.dst_expert_stride);
    e.dst_stride = j.dst_expert_stride * des;
    e.src = static_cast<const uint8_t*>(j.src), e.dst = static_cast<uint8_t*>(j.dst);
    e.upe = (uint32_t)upe, e.kind = (int16_t)j.kind, e.out_dtype = (int16_t)j.out_dtype;
    units = upe * j.E;
    return GQ_OK;
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_level_switch_experts(const gq_switch_experts_job_t* jobs_host, int n_jobs, void* stream) {
    if (int rc = options_ok()) return rc;
    if (n_jobs < 0) GQ_FAIL(GQ_E_BAD_SHAPE, WHO ": n_jobs=%d (n_jobs < 0)", n_jobs);
    if (n_jobs == 0) return GQ_OK;
    if (!jobs_host) GQ_FAIL(GQ_E_NULL, WHO ": jobs_host is NULL");
    ExpertsEntry e;
    int64_t units;
    for (int i = 0; i < n_jobs; ++i)  // all refusals first: a refused call has launched nothing
        if (int rc = check_job(jobs_host[i], i, e, units)) return rc;
    hipStream_t st = (hipStream_t)stream;
    ExpertsTable t;
    for (int i = 0; i < n_jobs;) {
        int64_t total = 0;
        t.n = 0, t.pad = 0;
        while (i < n_jobs && t.n < GQ_SWITCH_EXPERTS_MAX_JOBS) {
            check_job(jobs_host[i], i, t.e[t.n], units);
            if (total + units > MAX_UNITS) break;  // (a single job never exceeds it: checked above)
            total += units;
            t.e[t.n++].unit_end = (uint32_t)total;
            ++i;
        }
        for (int k = t.n; k < GQ_SWITCH_EXPERTS_MAX_JOBS; ++k) t.e[k] = ExpertsEntry{};
        hipLaunchKernelGGL(level_switch_experts_kernel, dim3((unsigned)total), dim3(256), 0, st, t);
        GQ_LAUNCH_CHECK();
    }
    return GQ_OK;
}

}  // extern "C"
