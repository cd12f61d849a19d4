/*
 * mg_cheby_coefs.h -- the factors of the KSPCHEBYSHEV recurrence (PETSc's classic three-term cheby.c; oracle/mgo.c), the ONE place they
 * are evaluated: the step-by-step smoother (mg_solver.c), the fused passes (mg_cheby.c), the tail kernel's launcher (libmgk.so) and the
 * host-memory stand-ins of the tests include it, so the bits cannot drift.  Header only: no symbol of either library.
 *
 *   scale = 2/(emax+emin) for the first step, p1 = p0 + scale*z(p0); then per step
 *   c_kp1 = 2 mu c_k - c_km1, omega = (2/alpha) c_k / c_kp1 and c3 = {1 - omega, omega, omega*Gamma*scale} with Gamma = 1:
 *   p_kp1 = (c3[0]*p_km1 + c3[1]*p_k) + c3[2]*z(p_k),  z(p) = (b - A p)*dinv
 */
#ifndef MG_CHEBY_COEFS_H
#define MG_CHEBY_COEFS_H
typedef struct mg_cheby_rec { double scale, mu, omegaprod, ckm1, ck; } mg_cheby_rec;
static inline void mg_cheby_begin(mg_cheby_rec *r, double emin, double emax) {
    const double scale = 2.0 / (emax + emin), alpha = 1.0 - scale * emin;
    r->scale = scale; r->mu = 1.0 / alpha; r->omegaprod = 2.0 / alpha; r->ckm1 = 1.0; r->ck = r->mu;
}
static inline void mg_cheby_next(mg_cheby_rec *r, double *c3) {
    const double Gamma = 1.0;
    const double ckp1 = 2.0 * r->mu * r->ck - r->ckm1;
    const double omega = r->omegaprod * r->ck / ckp1;
    c3[0] = 1.0 - omega; c3[1] = omega; c3[2] = omega * Gamma * r->scale;
    r->ckm1 = r->ck; r->ck = ckp1;
}
#endif
