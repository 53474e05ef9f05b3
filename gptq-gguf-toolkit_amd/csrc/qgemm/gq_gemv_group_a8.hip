// gq_gemv_group_a8.hip -- K39: the projections of one input of a dense decode step on int8 activations, in one launch.
//   gq_gemv_packed_group_a8  SPLIT: y_m = x W_m^T for up to four packed weights of one x (q / k / v), types mixed freely;
//                            SWIGLU: act = silu(x Wg^T) * (x Wu^T) for the gate / up pair of a dense MLP, G and U never written
//   gq_gemv_group_a8_plan    the LDS image and the partition of the grid: csrc/qgemm/gq_gemv_a8_plan.hpp
// The contract is include/gptq_gguf_qgemv_group_a8.h's.  K37's form (gq_gemv_a8.hip: the activation quantizer in the prologue,
// weights straight into registers, v_dot4_i32_i8 against the image in LDS, integer reductions over four lanes; a wave owns one
// row per turn and all of C) on a grid that is PARTITIONED among the members instead of launched once per member.
//
// Why.  A Llama / Qwen3 layer at T = 1 issued q, k, v as three launches, each quantizing the same x in 16 .. 256 workgroups;
// k and v of a grouped-query model (1024 rows at Llama-3-8B) are 64 workgroups, a quarter of the device.  Here every
// workgroup of ONE grid of at most 256 quantizes x once and then streams rows of the member it belongs to.
//
// SPLIT.  The host's plan (make_gemv_group_a8_plan: largest remainder on the members' weight bytes, each member at least one
// workgroup and at most one per row group of 16) is copied into the kernel's arguments with the members' pointers: no device
// table.  Workgroup b finds its member m by comparing b with the at most three inner boundaries first_wg[1 .. n - 1] -- scalar
// compares on kernel arguments, uniform over the workgroup -- and is workgroup lb = b - first_wg[m] of the member's g_m.  It
// switches ONCE on the member's type into member_walk<QT, TT>: the loads of the wave's first row (in flight during the
// prologue), gemva8::quantize_image, the kernel's only barrier, then gemva8::row_walk over row groups lb, lb + g_m, ..  The
// kernel is instantiated per TT (the host knows T); the switch over the six types is per workgroup, so one launch mixes types
// (Q4_K_M files keep v in Q6_K beside q and k in Q4_K).  The walk and the image are K37's text, so member m's row r is bit for
// bit gq_gemv_packed_a8's: a row's bits depend on its row and on x only.
//
// SWIGLU.  Gate and up have one type (the entry point requires it; the Python layer serves a mixed pair with SPLIT and
// gq_fwd_silu_mul), so the host knows it and the kernel is instantiated per <QT, TT>: no switch, and the registers of one
// type's walk only.  A wave walks VIRTUAL rows v = 2 r (gate row r) and v = 2 r + 1 (up row r) back to back through the same
// pipelined loads: row_at picks the tensor by v & 1 and next goes v -> v + 1 -> v + 2 * stride - 1.  At the end of a gate row
// lane t keeps token t's sum, rounded once to the activation dtype, in a register; at the end of the up row it rounds that
// sum once as well and stores a8core::silu_mul_rounded(g, u) -- gq_fwd_silu_mul's two roundings -- to act[t, r].  No LDS, no
// further barrier, and the [T, I] gate and up results never exist in memory.
//
// No atomics, no workspace, no scratch memory of the launch's own, no host synchronisation; plain vector stores.
#include "../../../include/gptq_gguf_qgemv_group_a8.h"

#include <atomic>

#include "../search/gq_block_host.hpp"
#include "gq_gemv_a8_core.hpp"

namespace gq {
namespace {

using namespace gemva8;

struct GroupMember {
    const uint8_t* blocks;
    const int32_t* row_src;
    uint16_t* y;
    int R;   // < 2^31 (check_R)
    int qt;
};
// the kernel's argument: the members and the partition of the grid, first_wg[m] .. first_wg[m + 1] - 1 are member m's
struct GroupTable {
    GroupMember m[GEMV_GROUP_A8_MAX];
    int first_wg[GEMV_GROUP_A8_MAX + 1];
    int n;
};

// workgroup lb of the nwg that member `me` owns: first loads, the prologue, the barrier, the walk
template <int QT, int TT>
__device__ __forceinline__ void member_walk(const GroupMember& me, int lb, int nwg, int C, const uint16_t* __restrict__ x, int bf16,
                                            uint8_t* a8_img) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), p = lane & 3, g4 = lane >> 2;
    const int nsb = C / 256;
    const int64_t R = me.R;
    const int32_t* __restrict__ row_src = me.row_src;
    auto row_at = rows_of<QT>(me.blocks, [=](int64_t r) { return row_src ? (int64_t)row_src[r] : r; }, nsb);

    const int64_t r = (int64_t)lb * GEMV_A8_ROWS + wave;
    uint32_t cur[NRAW<QT>] = {};
    if (r < R) load_item<QT>(row_at, nsb, g4, p, cur, r, 0);  // in flight during the prologue

    quantize_image(TT, TT * nsb, C, [](int sbi) { return (int64_t)sbi * 256; }, x, nullptr, bf16, a8_img);
    __syncthreads();

    row_walk<QT, TT>(row_at, R, C, r, rows_apart((int64_t)nwg * GEMV_A8_ROWS), cur, a8_img,
                     store_rows(me.y, R, bf16, [](int t) { return t; }));
}

template <int TT>
__global__ __launch_bounds__(NT) void gemv_group_a8_kernel(const GroupTable tab, int C, const uint16_t* __restrict__ x, int bf16) {
    extern __shared__ __attribute__((aligned(16))) uint8_t a8_img[];
    const int b = blockIdx.x;
    int m = 0;  // the member whose range holds b: scalar compares on the arguments
#pragma unroll
    for (int u = 1; u < GEMV_GROUP_A8_MAX; ++u) m += (u < tab.n && b >= tab.first_wg[u]) ? 1 : 0;
    const GroupMember me = tab.m[m];
    const int lb = b - tab.first_wg[m], nwg = tab.first_wg[m + 1] - tab.first_wg[m];
    switch (me.qt) {  // uniform over the workgroup
    case GQ_Q2_K: member_walk<GQ_Q2_K, TT>(me, lb, nwg, C, x, bf16, a8_img); break;
    case GQ_Q3_K: member_walk<GQ_Q3_K, TT>(me, lb, nwg, C, x, bf16, a8_img); break;
    case GQ_Q4_K: member_walk<GQ_Q4_K, TT>(me, lb, nwg, C, x, bf16, a8_img); break;
    case GQ_Q5_K: member_walk<GQ_Q5_K, TT>(me, lb, nwg, C, x, bf16, a8_img); break;
    case GQ_Q6_K: member_walk<GQ_Q6_K, TT>(me, lb, nwg, C, x, bf16, a8_img); break;
    default: member_walk<GQ_Q8_0, TT>(me, lb, nwg, C, x, bf16, a8_img); break;
    }
}

template <int QT, int TT>
__global__ __launch_bounds__(NT) void gemv_swiglu_a8_kernel(const uint8_t* __restrict__ gate, const int32_t* __restrict__ gate_src,
                                                           const uint8_t* __restrict__ up, const int32_t* __restrict__ up_src,
                                                           int64_t R, int C, const uint16_t* __restrict__ x, int bf16,
                                                           uint16_t* __restrict__ act) {
    extern __shared__ __attribute__((aligned(16))) uint8_t a8_img[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), p = lane & 3, g4 = lane >> 2;
    const int nsb = C / 256;
    // virtual row v: row v >> 1 of gate (v even) or of up (v odd)
    auto row_at = [=](int64_t v) {
        const int64_t r = v >> 1;
        const uint8_t* B = (v & 1) ? up : gate;
        const int32_t* src = (v & 1) ? up_src : gate_src;
        return B + (src ? (int64_t)src[r] : r) * nsb * ROWB<QT>;
    };
    const int64_t stride = (int64_t)gridDim.x * GEMV_A8_ROWS;
    auto next = [=](int64_t v) { return (v & 1) ? v + 2 * stride - 1 : v + 1; };

    const int64_t v0 = 2 * ((int64_t)blockIdx.x * GEMV_A8_ROWS + wave);
    uint32_t cur[NRAW<QT>] = {};
    if (v0 < 2 * R) load_item<QT>(row_at, nsb, g4, p, cur, v0, 0);  // in flight during the prologue

    quantize_image(TT, TT * nsb, C, [](int sbi) { return (int64_t)sbi * 256; }, x, nullptr, bf16, a8_img);
    __syncthreads();

    float g = 0.f;  // lane t: token t's gate value of the row in hand, rounded to the activation dtype
    row_walk<QT, TT>(row_at, 2 * R, C, v0, next, cur, a8_img, [&](int t, int64_t v, float s) {
        if (lane != t) return;
        const float q = bf16 ? bf2f(f2bf(s)) : h2f(f2h(s));  // G, U: what gq_gemv_packed_a8 would have stored
        if (!(v & 1)) g = q;
        else act[(int64_t)t * R + (v >> 1)] = bf16 ? f2bf(silu_mul_rounded<true>(g, q)) : f2h(silu_mul_rounded<false>(g, q));
    });
}

template <class K>
int allow_lds(K kernel, std::atomic<bool>& attr_set) {
    if (!attr_set) {
        GQ_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEMV_A8_LDS_BUDGET));
        attr_set = true;
    }
    return GQ_OK;
}

template <int TT>
int launch_split(const GemvGroupA8Plan& pl, const GroupTable& tab, int64_t C, const uint16_t* x, int bf16, hipStream_t st) {
    static std::atomic<bool> attr_set{false};
    if (int rc = allow_lds(gemv_group_a8_kernel<TT>, attr_set)) return rc;
    hipLaunchKernelGGL((gemv_group_a8_kernel<TT>), dim3((unsigned)pl.grid), dim3(NT), (size_t)pl.lds_bytes, st, tab, (int)C, x, bf16);
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

template <int QT, int TT>
int launch_swiglu(const GemvGroupA8Plan& pl, const GroupTable& tab, int64_t C, const uint16_t* x, int bf16, hipStream_t st) {
    static std::atomic<bool> attr_set{false};
    if (int rc = allow_lds(gemv_swiglu_a8_kernel<QT, TT>, attr_set)) return rc;
    hipLaunchKernelGGL((gemv_swiglu_a8_kernel<QT, TT>), dim3((unsigned)pl.grid), dim3(NT), (size_t)pl.lds_bytes, st, tab.m[0].blocks,
                       tab.m[0].row_src, tab.m[1].blocks, tab.m[1].row_src, (int64_t)tab.m[0].R, (int)C, x, bf16, tab.m[0].y);
    GQ_LAUNCH_CHECK();
    return GQ_OK;
}

// f(std::integral_constant<int, T>{}) for 1 <= T <= 4
template <class F>
void dispatch_tokens(int64_t T, F&& f) {
    switch (T) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
    }
}

// ---- the checks the call and its plan share, in the header's order
int check_mode_n(const char* who, int mode, int n) {
    if (mode != GQ_GEMV_GROUP_SPLIT && mode != GQ_GEMV_GROUP_SWIGLU)
        GQ_FAIL(GQ_E_BAD_TYPE, "%s: mode %d (GQ_GEMV_GROUP_SPLIT or GQ_GEMV_GROUP_SWIGLU)", who, mode);
    if (n < 1 || n > GQ_GEMV_GROUP_MAX) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: n_members=%d (not in [1, %d])", who, n, GQ_GEMV_GROUP_MAX);
    return GQ_OK;
}
int check_member_types(const char* who, const int* qt, int n, int mode) {
    for (int m = 0; m < n; ++m) {
        if (qt[m] == GQ_IQ4_NL || qt[m] == GQ_IQ4_XS)
            GQ_FAIL(GQ_E_BAD_TYPE, "%s: members[%d].q_type %d (%s) is not served on int8 activations (a K-quant or GQ_Q8_0)", who, m,
                    qt[m], qt[m] == GQ_IQ4_NL ? "GQ_IQ4_NL" : "GQ_IQ4_XS");
        if (!a8_type(qt[m])) GQ_FAIL(GQ_E_BAD_TYPE, "%s: members[%d].q_type: unknown q_type %d (a K-quant or GQ_Q8_0)", who, m, qt[m]);
    }
    if (mode == GQ_GEMV_GROUP_SWIGLU) {
        if (n != 2) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: n_members=%d (GQ_GEMV_GROUP_SWIGLU takes exactly 2: gate, up)", who, n);
        if (qt[1] != qt[0])
            GQ_FAIL(GQ_E_BAD_TYPE, "%s: members[1].q_type %d != members[0].q_type %d (GQ_GEMV_GROUP_SWIGLU takes one type)", who, qt[1], qt[0]);
    }
    return GQ_OK;
}
int check_member_sizes(const char* who, const int64_t* R, int n, int64_t C, int64_t T, int mode) {
    for (int m = 0; m < n; ++m)
        if (R[m] < 1 || R[m] > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: members[%d].R=%ld (not in [1, 2^31))", who, m, (long)R[m]);
    if (mode == GQ_GEMV_GROUP_SWIGLU && R[1] != R[0])
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: members[1].R=%ld != members[0].R=%ld (GQ_GEMV_GROUP_SWIGLU takes one shape)", who, (long)R[1], (long)R[0]);
    if (T < 1 || T > GQ_GEMV_A8_MAX_T) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: T=%ld (not in [1, %d])", who, (long)T, GQ_GEMV_A8_MAX_T);
    return check_C256(who, C);
}
GemvGroupA8Plan plan_of(const int* qt, const int64_t* R, int n, int64_t C, int64_t T, int mode) {
    int64_t row_bytes[GEMV_GROUP_A8_MAX];
    for (int m = 0; m < n; ++m) row_bytes[m] = C / block_geometry(qt[m]).bs * block_geometry(qt[m]).ts;
    return make_gemv_group_a8_plan(R, row_bytes, n, C, T, mode == GQ_GEMV_GROUP_SWIGLU);
}

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

int gq_gemv_group_a8_plan(const int* q_types, const int64_t* R, int n_members, int64_t C, int64_t T, int mode, int64_t* lds_bytes,
                          int64_t* grid, int64_t* first_wg, int64_t* fits) {
    const char* who = "gq_gemv_group_a8_plan";
    if (int rc = check_mode_n(who, mode, n_members)) return rc;
    if (int rc = need(who, "q_types", q_types)) return rc;
    if (int rc = need(who, "R", R)) return rc;
    if (int rc = check_member_types(who, q_types, n_members, mode)) return rc;
    if (int rc = check_member_sizes(who, R, n_members, C, T, mode)) return rc;
    const GemvGroupA8Plan p = plan_of(q_types, R, n_members, C, T, mode);
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    if (grid) *grid = p.grid;
    if (first_wg)
        for (int m = 0; m <= n_members; ++m) first_wg[m] = p.first_wg[m];
    if (fits) *fits = p.fits;
    return GQ_OK;
}

int gq_gemv_packed_group_a8(const gq_gemv_member_t* members, int n_members, int64_t C, const void* x, int64_t T, int x_dtype, int mode,
                            void* stream) {
    if (int rc = options_ok()) return rc;
    const char* who = "gq_gemv_packed_group_a8";
    const bool swiglu = mode == GQ_GEMV_GROUP_SWIGLU;
    if (int rc = check_mode_n(who, mode, n_members)) return rc;
    if (int rc = need(who, "members", members)) return rc;
    if (x_dtype != GQ_F16 && x_dtype != GQ_BF16)
        GQ_FAIL(GQ_E_BAD_TYPE, "%s: x_dtype %d (GQ_F16 or GQ_BF16; there is no fp32 path)", who, x_dtype);
    int qt[GEMV_GROUP_A8_MAX];
    int64_t R[GEMV_GROUP_A8_MAX];
    for (int m = 0; m < n_members; ++m) qt[m] = members[m].q_type, R[m] = members[m].R;
    if (int rc = check_member_types(who, qt, n_members, mode)) return rc;
    if (swiglu && members[1].y) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: members[1].y is not NULL (GQ_GEMV_GROUP_SWIGLU writes members[0].y only)", who);
    char name[32];
    auto field = [&](int m, const char* f) { return snprintf(name, sizeof name, "members[%d].%s", m, f), name; };
    for (int m = 0; m < n_members; ++m) {
        if (int rc = need(who, field(m, "blocks"), members[m].blocks)) return rc;
        if (!(swiglu && m == 1))
            if (int rc = need(who, field(m, "y"), members[m].y)) return rc;
    }
    if (int rc = need(who, "x", x)) return rc;
    if (int rc = check_member_sizes(who, R, n_members, C, T, mode)) return rc;
    const GemvGroupA8Plan pl = plan_of(qt, R, n_members, C, T, mode);
    if (!pl.fits)
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: T=%ld C=%ld: the quantized image of x, %ld bytes, does not fit the %ld bytes of LDS it may take",
                who, (long)T, (long)C, (long)pl.lds_bytes, (long)GEMV_A8_LDS_BUDGET);
    for (int m = 0; m < n_members; ++m) {
        if (int rc = check_aligned(who, field(m, "blocks"), members[m].blocks, block_align(qt[m]))) return rc;
        if (int rc = check_aligned(who, field(m, "row_src"), members[m].row_src, 4)) return rc;
        if (int rc = check_aligned(who, field(m, "y"), members[m].y, 16)) return rc;
    }
    if (int rc = check_aligned(who, "x", x, 16)) return rc;

    GroupTable tab{};
    tab.n = n_members;
    for (int m = 0; m < n_members; ++m)
        tab.m[m] = {static_cast<const uint8_t*>(members[m].blocks), members[m].row_src, static_cast<uint16_t*>(members[m].y), (int)R[m], qt[m]};
    for (int m = 0; m <= n_members; ++m) tab.first_wg[m] = (int)pl.first_wg[m];
    const uint16_t* xs = static_cast<const uint16_t*>(x);
    const int bf16 = x_dtype == GQ_BF16;
    int rc = GQ_OK;
    dispatch_tokens(T, [&](auto tt) {
        constexpr int TT = decltype(tt)::value;
        if (!swiglu) {
            rc = launch_split<TT>(pl, tab, C, xs, bf16, (hipStream_t)stream);
            return;
        }
        dispatch_packed(qt[0], [&](auto q) {
            constexpr int QT = decltype(q)::value;
            if constexpr (a8_type(QT)) rc = launch_swiglu<QT, TT>(pl, tab, C, xs, bf16, (hipStream_t)stream);
        });
    });
    return rc;
}

}  // extern "C"
