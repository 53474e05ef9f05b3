// gq_rsqrt_rn.hpp -- the correctly rounded fp32 1 / sqrt(x) of the order-matched norm kernels: what torch.rsqrt returns on
// this stack.  The text of gq_forward.hip's rsqrt_rn (gq_fwd_rmsnorm_ordered), restated for the kernels under forward/: that
// file is one of the top-level sources whose hash the committed traffic records pin (tests/test_block_layout_cpu.py), so
// the function was not moved out of it.
#pragma once
#include "../gq_common.hpp"

namespace gq {

// Correctly rounded 1 / sqrt(x) in fp32 (what torch.rsqrt returns on this stack: 0 differences in 4 M samples against the
// double-precision value rounded once; v_rsq_f32 alone is a 1-ulp approximation).  The double-precision estimate rounded to
// fp32 is right unless 1 / sqrt(x) lies within 2^-53 of a rounding boundary; the boundaries y -+ ulp / 2 are tested exactly:
// (y +- h)^2 has <= 50 significant bits (exact in double), its product with x is taken as an unevaluated sum t + e (fma).
__device__ __forceinline__ float rsqrt_rn(float x) {
    float y = (float)(1.0 / sqrt((double)x));
    if (!(x > 0.0f) || !(y > 0.0f) || y > 3.0e38f) return y;  // zero / negative / nan / overflow: nothing to repair
    // product (m * m) * x compared with 1, exactly
    auto above_one = [](double m, double xd) {  // m^2 x > 1 ?
        const double p = m * m;                 // exact
        const double t = p * xd, e = fma(p, xd, -t);
        return t > 1.0 || (t == 1.0 && e > 0.0);
    };
    auto below_one = [](double m, double xd) {  // m^2 x < 1 ?
        const double p = m * m;
        const double t = p * xd, e = fma(p, xd, -t);
        return t < 1.0 || (t == 1.0 && e < 0.0);
    };
    const float up = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, y) + 1u);
    const float dn = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, y) - 1u);
    const double hi = 0.5 * ((double)y + (double)up), lo = 0.5 * ((double)y + (double)dn);  // the rounding boundaries
    // 1 / sqrt(x) > hi  <=>  hi^2 x < 1: the neighbour above is closer; 1 / sqrt(x) < lo  <=>  lo^2 x > 1: the one below
    // (on a boundary exactly -- impossible for 1 / sqrt of a float other than a power of four -- y stays)
    if (below_one(hi, (double)x)) return up;
    if (above_one(lo, (double)x)) return dn;
    return y;
}

}  // namespace gq
