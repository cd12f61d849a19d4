/* mgk_pow2.h -- the host predicate of the exact-FMA stencil form, in plain C so that the launch rules (mgk_launch.hpp) and
 * the CPU test of the rule (tests/exact_fma_check.c) read the same text.
 * A coefficient a = +-2^e with e >= 0 makes every product a * x exact as long as it does not overflow: a binary scaling that only raises
 * the exponent, subnormal x included.  fma(a, x, t) then rounds the same real number as t + (a * x) and is the same double.  Below 1 the
 * product of a subnormal x loses bits, so those coefficients -- like zeros, infinities, NaN and everything with more than one mantissa
 * bit -- are "not exact" and keep the generic form. */
#ifndef MGK_POW2_H
#define MGK_POW2_H
#include <math.h>
static inline int mgk_coef_exact_pow2(double a) {
    int e = 0;
    if (!(a == a) || a == 0.0 || a - a != 0.0) return 0;      /* NaN, zero, +-inf (frexp leaves the exponent unspecified for them) */
    const double m = frexp(a, &e);
    return (m == 0.5 || m == -0.5) && e >= 1;                 /* |a| = 0.5 * 2^e = 2^(e-1) with e - 1 >= 0 */
}
/* bit k set: coef[k] of a stencil of n coefficients is exact (the centre included if it happens to be) */
static inline unsigned mgk_coef_exact_mask(const double *coef, int n) {
    unsigned m = 0;
    for (int k = 0; k < n; k++) if (mgk_coef_exact_pow2(coef[k])) m |= 1u << k;
    return m;
}
#endif
