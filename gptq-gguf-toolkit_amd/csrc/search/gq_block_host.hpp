// gq_block_host.hpp -- the host side of the packed block types (K-quants, Q8_0, IQ4_NL, IQ4_XS): the ONE list of the types,
// their alignment and geometry read from the layout structs of gq_block_decode.hpp, the turn of a run-time flag into a
// template argument, and the operand checks the four packed matmul entry points share.  Host code only; included by
// decode/gq_decode.hip, search/gq_switch.hip and the four qgemm/*.hip files.  A new block type is added to dispatch_packed
// (and to the layout structs): every entry point then accepts it, and none can fall into another type's kernel.
#pragma once
#include <type_traits>

#include "gq_block_decode.hpp"

namespace gq {
namespace blockdec {

// f(std::integral_constant<int, QT>{}) for the packed type q_type -> true; any other q_type: nothing is called -> false.
// (The order of the cases is the order in which a file's kernels are instantiated and so laid out in its code object.)
template <class F>
constexpr bool dispatch_packed(int q_type, F&& f) {
    switch (q_type) {
    case GQ_Q2_K: f(std::integral_constant<int, GQ_Q2_K>{}); return true;
    case GQ_Q3_K: f(std::integral_constant<int, GQ_Q3_K>{}); return true;
    case GQ_Q4_K: f(std::integral_constant<int, GQ_Q4_K>{}); return true;
    case GQ_Q5_K: f(std::integral_constant<int, GQ_Q5_K>{}); return true;
    case GQ_Q6_K: f(std::integral_constant<int, GQ_Q6_K>{}); return true;
    case GQ_IQ4_NL: f(std::integral_constant<int, GQ_IQ4_NL>{}); return true;
    case GQ_IQ4_XS: f(std::integral_constant<int, GQ_IQ4_XS>{}); return true;
    case GQ_Q8_0: f(std::integral_constant<int, GQ_Q8_0>{}); return true;
    default: return false;
    }
}

// f(std::true_type{}) or f(std::false_type{}): a flag (bf16, the wide tile) as a template argument of the launch
template <class F>
inline void dispatch_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// the types whose blocks the GPU reads
constexpr bool packed_type(int q) { return dispatch_packed(q, [](auto) {}); }

// values and bytes of a block: the 32-value types are those that have a Lay32
template <int QT, class = void> struct Geo { static constexpr int BS = 256, TS = Lay<QT>::TS; };
template <int QT> struct Geo<QT, std::void_t<decltype(Lay32<QT>::TS)>> { static constexpr int BS = 32, TS = Lay32<QT>::TS; };
struct Geometry { int bs, ts; };

constexpr Geometry block_geometry(int q) {  // {0, 0} for a type that is not packed
    Geometry g = {0, 0};
    dispatch_packed(q, [&](auto t) { g = {Geo<decltype(t)::value>::BS, Geo<decltype(t)::value>::TS}; });
    return g;
}
// the alignment of a block: the width of the staging loads (0 for a type that is not packed)
constexpr int block_align(int q) {
    int al = 0;
    dispatch_packed(q, [&](auto t) { al = QL<decltype(t)::value>::AL; });
    return al;
}
static_assert(block_align(GQ_Q2_K) == 4, "Q2_K");
static_assert(block_align(GQ_Q3_K) == 2, "Q3_K");
static_assert(block_align(GQ_Q4_K) == 16, "Q4_K");
static_assert(block_align(GQ_Q5_K) == 16, "Q5_K");
static_assert(block_align(GQ_Q6_K) == 2, "Q6_K");
static_assert(block_align(GQ_Q8_0) == 2, "Q8_0");
static_assert(block_align(GQ_IQ4_NL) == 2, "IQ4_NL");
static_assert(block_align(GQ_IQ4_XS) == 8, "IQ4_XS");
static_assert(block_geometry(GQ_Q8_0).bs == 32 && block_geometry(GQ_IQ4_NL).bs == 32 && block_geometry(GQ_Q6_K).bs == 256 &&
                  block_geometry(GQ_IQ4_XS).bs == 256 && !packed_type(GQ_F16) && block_align(9) == 0,
              "the 32-value types are Q8_0 and IQ4_NL; nothing else is packed");

// ---- the operand checks of gq_linear_packed, gq_gemv_packed, gq_gemv_packed_experts and gq_linear_packed_experts: `who` is
// the entry point's name.  Each returns GQ_OK or sets the message and returns the status; an entry point lists them in its
// documented order between its own checks, all of them before its first HIP call.
inline int check_types(const char* who, int q_type, int x_dtype) {
    if (!packed_type(q_type)) GQ_FAIL(GQ_E_BAD_TYPE, "%s: unknown q_type %d (a K-quant, GQ_Q8_0, GQ_IQ4_NL or GQ_IQ4_XS)", who, q_type);
    if (x_dtype != GQ_F16 && x_dtype != GQ_BF16)
        GQ_FAIL(GQ_E_BAD_TYPE, "%s: x_dtype %d (GQ_F16 or GQ_BF16; there is no fp32 path)", who, x_dtype);
    return GQ_OK;
}
inline int need(const char* who, const char* name, const void* p) {
    if (!p) GQ_FAIL(GQ_E_NULL, "%s: %s is NULL", who, name);
    return GQ_OK;
}
inline int check_R(const char* who, int64_t R) {
    if (R < 1 || R > 0x7fffffff) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: R=%ld (not in [1, 2^31))", who, (long)R);
    return GQ_OK;
}
inline int check_C256(const char* who, int64_t C) {
    if (C < 256 || C > 0x7fffffff || C % 256)
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: C=%ld (C %% 256 != 0 or not in [256, 2^31); Q8_0 and IQ4_NL included)", who, (long)C);
    return GQ_OK;
}
// the pairs of a grouped call: P = x_rows * pairs_per_row (P in range: checked by the caller)
inline int check_pairs(const char* who, int64_t x_rows, int64_t pairs_per_row, int64_t P) {
    if (pairs_per_row < 1 || x_rows < 1 || pairs_per_row > P || x_rows > P || x_rows * pairs_per_row != P)
        GQ_FAIL(GQ_E_BAD_SHAPE, "%s: x_rows=%ld * pairs_per_row=%ld != P=%ld", who, (long)x_rows, (long)pairs_per_row, (long)P);
    return GQ_OK;
}
inline int check_aligned(const char* who, const char* name, const void* p, int a) {
    if (!aligned(p, a)) GQ_FAIL(GQ_E_BAD_SHAPE, "%s: %s not %d-byte aligned", who, name, a);
    return GQ_OK;
}
inline int check_blocks_aligned(const char* who, int q_type, const void* blocks) {
    return check_aligned(who, "blocks", blocks, block_align(q_type));
}

}  // namespace blockdec
}  // namespace gq
