/* exact_fma_check.c -- CPU check of the exact-FMA rule of the fp64 stencil kernels (csrc/mgk_pow2.h, madd in
 * csrc/mgk_dev.hpp).  Build with -ffp-contract=off, so that "t + a * x" below is a multiply and an add, as in the kernels' generic form.
 *   1. the host predicate mgk_coef_exact_pow2 on the values the rule names;
 *   2. the canonical 7-term sum t = a0 x0; t = t + ak xk evaluated both ways -- the six off-diagonal terms as multiply + add and as
 *      fma(ak, xk, t), the first product and the centre term never fused -- on random tuples: the same bits, memcmp.
 * usage: exact_fma_check [tuples per coefficient]   (default 300000: 1.2e6 tuples over the four coefficients) */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mgk_pow2.h"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL: "); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng(void) {                                    /* xorshift64* */
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}
static double unit(void) { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }
/* magnitudes log-uniform over 1e-320 .. 1e300 (subnormals included), either sign; one value in sixteen is +0 or -0 */
static double draw(void) {
    const uint64_t r = rng();
    if ((r & 15u) == 0) return (r & 16u) ? -0.0 : 0.0;
    const double mag = pow(10.0, -320.0 + 620.0 * unit()) * (0.5 + unit());
    return (r & 32u) ? -mag : mag;
}

static void check_predicate(void) {
    for (int e = 0; e <= 60; e++) {
        CHECK(mgk_coef_exact_pow2(ldexp(1.0, e)) == 1, "2^%d must be exact", e);
        CHECK(mgk_coef_exact_pow2(-ldexp(1.0, e)) == 1, "-2^%d must be exact", e);
    }
    CHECK(mgk_coef_exact_pow2(0.5) == 0, "0.5 (e < 0) is not exact");
    CHECK(mgk_coef_exact_pow2(0.25) == 0 && mgk_coef_exact_pow2(-0.5) == 0, "0.25, -0.5 are not exact");
    CHECK(mgk_coef_exact_pow2(3.0 * 1048576.0) == 0, "3 * 2^20 is not exact");
    CHECK(mgk_coef_exact_pow2(3.0 * 1024.0) == 0 && mgk_coef_exact_pow2(1.0 + DBL_EPSILON) == 0, "two mantissa bits are not exact");
    CHECK(mgk_coef_exact_pow2(0.0) == 0 && mgk_coef_exact_pow2(-0.0) == 0, "zero is not exact");
    CHECK(mgk_coef_exact_pow2(INFINITY) == 0 && mgk_coef_exact_pow2(-INFINITY) == 0, "inf is not exact");
    CHECK(mgk_coef_exact_pow2(NAN) == 0, "NaN is not exact");
    CHECK(mgk_coef_exact_pow2(DBL_MIN) == 0, "the smallest normal is not exact");
    CHECK(mgk_coef_exact_pow2(4.9406564584124654e-324) == 0 && mgk_coef_exact_pow2(DBL_MIN / 4.0) == 0, "subnormals are not exact");
    CHECK(mgk_coef_exact_pow2(ldexp(1.0, 1023)) == 1, "2^1023 is exact (the rule's limit is the product, not the coefficient)");
    const double lap[7] = {1048576.0, 1048576.0, 1048576.0, -6.0 * 1048576.0, 1048576.0, 1048576.0, 1048576.0};
    CHECK((mgk_coef_exact_mask(lap, 7) & 0x77u) == 0x77u, "the Laplacian of the 1025^3 grid: all six off-diagonals exact");
    CHECK((mgk_coef_exact_mask(lap, 7) & 0x08u) == 0, "its centre -6 * 2^20 is not");
    const double mix[7] = {4.0, 16.0, 64.0, -168.0, 3072.0, 16.0, 4.0};
    CHECK(mgk_coef_exact_mask(mix, 7) == 0x67u, "3 * 2^10 at j+1 clears its bit only (mask %x)", mgk_coef_exact_mask(mix, 7));
}

static double sum_generic(const double *a, const double *x) {
    double t = a[0] * x[0];
    for (int k = 1; k < 7; k++) t = t + a[k] * x[k];
    return t;
}
static double sum_exact(const double *a, const double *x) {
    double t = a[0] * x[0];                                     /* the first product is never fused */
    for (int k = 1; k < 7; k++) t = (k == 3) ? t + a[k] * x[k] : fma(a[k], x[k], t);      /* nor is the centre term */
    return t;
}

int main(int argc, char **argv) {
    const long per = argc > 1 ? atol(argv[1]) : 300000;
    check_predicate();
    const double cs[4] = {1.0, 4.0, 1048576.0, -1024.0};
    long n = 0, nsub = 0, nzero = 0;
    for (int ci = 0; ci < 4; ci++) {
        const double c = cs[ci];
        const double a[7] = {c, c, c, -6.0 * c, c, c, c};
        CHECK((mgk_coef_exact_mask(a, 7) & 0x77u) == 0x77u, "c = %g: the launcher would take the exact form", c);
        for (long i = 0; i < per; i++, n++) {
            double x[7];
            for (int k = 0; k < 7; k++) x[k] = draw();
            /* every fourth tuple: all magnitudes within a few binades of each other, so that the terms cancel and round */
            if ((i & 3) == 0) { const double s = fabs(x[0]) > 0.0 ? x[0] : 1.0; for (int k = 1; k < 7; k++) x[k] = s * (unit() - 0.5) * 4.0; }
            const double g = sum_generic(a, x), f = sum_exact(a, x);
            if (g != 0.0 && fabs(g) < DBL_MIN) nsub++;
            if (g == 0.0) nzero++;
            CHECK(memcmp(&g, &f, sizeof g) == 0, "c = %g tuple %ld: generic %a, exact-FMA %a", c, i, g, f);
        }
    }
    printf("%s: %ld tuples (%ld subnormal sums, %ld zero sums), %d failures\n", fails ? "FAILED" : "ok", n, nsub, nzero, fails);
    return fails ? 1 : 0;
}
