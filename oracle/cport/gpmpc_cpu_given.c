/* TEST INFRASTRUCTURE ONLY -- one moment-matching step and the whole rollout, diagonal and full covariance, on GIVEN
 * per-data constants: beta [ds][N] and the folded pair weights M as GPPack.beta() / GPPack.weights() export them
 * (element (i <= j) at [a][j][i], row stride Np; sf^4, exp(-1/4 d^2) and the factor 2 of the off-diagonal pairs folded
 * in).  Nothing of the pack build is recomputed here, so its rounding stays out of a comparison with the HIP kernels,
 * which read the same numbers: what is left is the arithmetic of one step.
 *
 * Written from gpmpc_cpu_ld.c (diagonal step: the same operations in the same order) and gpmpc_cpu_fullcov.c (full
 * covariance step and cost, src/mpc.py:179-198: x_ref, u_ref, general Q, R, gamma, gamma = 0 included).  Type-generic
 * like the latter; compiled four times:
 *     (nothing)        double                 _d        the plain fp64 evaluation of the reference formula: K_ref
 *     -DLDBL           long double            _ld       the yardstick (x87, 64-bit significand)
 *     -DCPLX           double complex         _cd       complex-step gradient, the fp64 floor of cost and gradient
 *     -DLDBL -DCPLX    long double complex    _cld      complex-step gradient of the yardstick
 * The constants are fp64 numbers converted element by element where they are used (no long double copy of an N^2
 * matrix); with cld != 0 they are long double arrays instead, which only the pin against gpmpc_cpu_rollout_ld uses
 * (gpmpc_given_constants_ld builds them exactly as gpmpc_cpu_ld.c does).
 *
 * Next to every mean, variance and covariance the real builds return the sum of the ABSOLUTE values of the terms it was
 * formed from:
 *     A_mean = (sf^2 / sqrt(det_m)) sum_i |beta_i| l_i
 *     A_var  = sf^2 + c sum_(i<=j) |M_ij| E_ij + m^2
 *     A_cov  = c_ab sum_ij |beta_a,i beta_b,j| E_ij + |m_a m_b|            (a != b)
 *     A_exp  = c sum_(i<=j) |M_ij| E_ij (q_i + q_j + 2 sum_k |h_ik h_jk|)  (diagonal step: see step_diag)
 * 2^-53 A is the unit a rounding error of such a sum is measured in. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <complex.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define MAXD 8

#ifdef LDBL
typedef long double real;
#define R_ABS fabsl
#else
typedef double real;
#define R_ABS fabs
#endif

#if defined(LDBL) && defined(CPLX)
typedef long double complex num;
#define N_EXP cexpl
#define N_SQRT csqrtl
#define N_LOG clogl
#define N_ABS cabsl
#define FN(name) name##_cld
#elif defined(CPLX)
typedef double complex num;
#define N_EXP cexp
#define N_SQRT csqrt
#define N_LOG clog
#define N_ABS cabs
#define FN(name) name##_cd
#elif defined(LDBL)
typedef long double num;
#define N_EXP expl
#define N_SQRT sqrtl
#define N_LOG logl
#define N_ABS fabsl
#define FN(name) name##_ld
#else
typedef double num;
#define N_EXP exp
#define N_SQRT sqrt
#define N_LOG log
#define N_ABS fabs
#define FN(name) name##_d
#endif

/* the absolute sums are returned by the real builds only */
#ifdef CPLX
#define E_ABS(x) ((real)0.0)
#else
#define E_ABS(x) N_ABS(x)
#endif

typedef struct {
    int N, Np, ds, da, D, H;
    const double *X, *lam, *sf;
    const void *beta, *M;    /* [ds][N] and [ds][Np][Np], double (cld = 0) or long double */
    int cld;
    double gamma; const double *Q, *R, *xref, *uref;
    const double *init_cov, *action_var, *process_var;    /* noise model, each NULL = the constants below */
} ctx_t;

static inline real FN(cb)(const ctx_t* c, int a, int i) {
    const size_t k = (size_t)a * c->N + i;
    return c->cld ? (real)((const long double*)c->beta)[k] : (real)((const double*)c->beta)[k];
}
/* the pair (i <= j) */
static inline real FN(cm)(const ctx_t* c, int a, int i, int j) {
    const size_t k = ((size_t)a * c->Np + j) * c->Np + i;
    return c->cld ? (real)((const long double*)c->M)[k] : (real)((const double*)c->M)[k];
}

/* Diagonal step for the input N(u, diag(s)): gpmpc_cpu_ld.c:51-82, operation by operation.  Am / Av / Ax may be NULL.
 * Ax = c sum |M_ij| E_ij (q_i + q_j + 2 sum_k |h_ik h_jk|), q = |h|^2: the terms weighted with the size of the EXPANDED exponent
 * q_i + q_j + 2 h_i.h_j the HIP pair kernels evaluate; 2^-53 Ax is what rounding that exponent costs.  rowz, rowa, rowx [N] scratch. */
static void FN(step_diag)(const ctx_t* c, const num* u, const num* s, num* mt, num* vt, real* Am, real* Av, real* Ax, num* rowz, real* rowa, real* rowx) {
    const int N = c->N, ds = c->ds, D = c->D;
    for (int a = 0; a < ds; ++a) {
        const double* la = c->lam + a * D; const real sf2 = (real)c->sf[a] * (real)c->sf[a];
        num Bk[MAXD], sc[MAXD], detm = (real)1.0, detv = (real)1.0;
        for (int k = 0; k < D; ++k) {
            Bk[k] = (real)1.0 / (s[k] + (real)la[k]);
            sc[k] = N_SQRT((real)0.125 / ((real)0.5 * (real)la[k] + s[k]));
            detm *= s[k] / (real)la[k] + (real)1.0; detv *= (real)2.0 * s[k] / (real)la[k] + (real)1.0;
        }
        const num cm = sf2 / N_SQRT(detm), cv = (real)1.0 / N_SQRT(detv);
        num S0 = (real)0.0; real A0 = (real)0.0;
        for (int i = 0; i < N; ++i) {
            num q = (real)0.0;
            for (int k = 0; k < D; ++k) { const num d = u[k] - (real)c->X[(size_t)i * D + k]; q += Bk[k] * d * d; }
            const num l = N_EXP((real)-0.5 * q);
            S0 += FN(cb)(c, a, i) * l; A0 += R_ABS(FN(cb)(c, a, i)) * E_ABS(l);
        }
        const num m = cm * S0;
#pragma omp parallel for schedule(dynamic, 8)
        for (int i = 0; i < N; ++i) {
            num hi[MAXD], z0 = (real)0.0; real a0 = (real)0.0, x0 = (real)0.0;
            for (int k = 0; k < D; ++k) hi[k] = sc[k] * (u[k] - (real)c->X[(size_t)i * D + k]);
            for (int j = i; j < N; ++j) {
                num ss = (real)0.0; real ex = (real)0.0;
                for (int k = 0; k < D; ++k) {
                    const num hj = sc[k] * (u[k] - (real)c->X[(size_t)j * D + k]); const num mm = hi[k] + hj; ss += mm * mm;
                    ex += E_ABS(hi[k]) * E_ABS(hi[k]) + E_ABS(hj) * E_ABS(hj) + (real)2.0 * E_ABS(hi[k]) * E_ABS(hj);
                }
                const num E = N_EXP(-ss); const real w = FN(cm)(c, a, i, j);
                z0 += w * E; a0 += R_ABS(w) * E_ABS(E); x0 += R_ABS(w) * E_ABS(E) * ex;
            }
            rowz[i] = z0; rowa[i] = a0; rowx[i] = x0;
        }
        num Z0 = (real)0.0; real AZ = (real)0.0, AX = (real)0.0;
        for (int i = 0; i < N; ++i) { Z0 += rowz[i]; AZ += rowa[i]; AX += rowx[i]; }
        mt[a] = m; vt[a] = sf2 - cv * Z0 - m * m;
        if (Am) Am[a] = N_ABS(cm) * A0;
        if (Av) Av[a] = sf2 + N_ABS(cv) * AZ + N_ABS(m) * N_ABS(m);
        if (Ax) Ax[a] = N_ABS(cv) * AX;
    }
}

/* In-place Gauss-Jordan on the n x (n + m) augmented matrix a (row stride ld): returns det of the left block, leaves
 * [I | left^-1 right].  Pivoting compares moduli. */
static num FN(gauss_jordan)(int n, int m, num* a, int ld) {
    num det = (real)1.0;
    for (int k = 0; k < n; ++k) {
        int piv = k; real best = N_ABS(a[k * ld + k]);
        for (int r = k + 1; r < n; ++r) if (N_ABS(a[r * ld + k]) > best) { best = N_ABS(a[r * ld + k]); piv = r; }
        if (piv != k) { for (int q = 0; q < n + m; ++q) { num t = a[k * ld + q]; a[k * ld + q] = a[piv * ld + q]; a[piv * ld + q] = t; } det = -det; }
        const num pv = a[k * ld + k]; det *= pv;
        for (int q = 0; q < n + m; ++q) a[k * ld + q] /= pv;
        for (int r = 0; r < n; ++r) if (r != k) { const num f = a[r * ld + k]; for (int q = 0; q < n + m; ++q) a[r * ld + q] -= f * a[k * ld + q]; }
    }
    return det;
}

static num FN(inv_det)(int n, const num* Min, num* inv) {
    num a[MAXD * 2 * MAXD];
    for (int r = 0; r < n; ++r) for (int q = 0; q < n; ++q) { a[r * 2 * n + q] = Min[r * n + q]; a[r * 2 * n + n + q] = (r == q) ? (real)1.0 : (real)0.0; }
    const num det = FN(gauss_jordan)(n, n, a, 2 * n);
    for (int r = 0; r < n; ++r) for (int q = 0; q < n; ++q) inv[r * n + q] = a[r * 2 * n + n + q];
    return det;
}

/* Full-covariance step for the input N(u, S): gpmpc_cpu_fullcov.c step(), with the folded weights read instead of
 * built and every operation in ``num``.  mt [ds], ct [ds][ds]; Amn [ds] and Ac [ds][ds] may be NULL.  V, AV, Z2: N x D scratch;
 * gq: 2N; rowz, rowa: N.  S is read as given (no symmetrisation: the HIP kernels read (S + S^T)/2, so their callers pass that).
 * bug != 0: the cross term of the reference's line :446, z2_i^T Am z1_j instead of z1_i^T Am z2_j (GPMPC_COV_BUG_COMPAT;
 * oracle/gpmpc_oracle.py::covariance_prop(bug_compatible=True)), evaluated for every ORDERED pair (a, b) as the HIP kernel does, so
 * ct[a][b] and ct[b][a] are two sums of their own; 0 keeps every bit of the consistent form.
 * Lout [ds][N] (real builds, may be NULL): l_i = c_m exp(-1/2 v_i^T B v_i), the second return value of mean_prop_torch (:335-336). */
static void FN(step_full)(const ctx_t* c, const num* u, const num* S, int bug, num* mt, num* ct, real* Amn, real* Ac, real* Lout, num* V, num* AV, num* gq, num* Z2, num* rowz, real* rowa) {
    const int N = c->N, ds = c->ds, D = c->D;
    for (int i = 0; i < N; ++i) for (int k = 0; k < D; ++k) V[(size_t)i * D + k] = u[k] - (real)c->X[(size_t)i * D + k];
    num mu[MAXD];
    for (int a = 0; a < ds; ++a) {
        const double* la = c->lam + a * D; const real sf2 = (real)c->sf[a] * (real)c->sf[a];
        num Mx[MAXD * MAXD], Bm[MAXD * MAXD], Am[MAXD * MAXD], tmp[MAXD * MAXD], dummy[MAXD * MAXD];
        for (int r = 0; r < D; ++r) for (int q = 0; q < D; ++q) { Mx[r * D + q] = S[r * D + q] + (r == q ? (real)la[r] : (real)0.0); tmp[r * D + q] = S[r * D + q] / (real)la[r] + (r == q ? (real)1.0 : (real)0.0); }
        FN(inv_det)(D, Mx, Bm);
        const num detm = FN(inv_det)(D, tmp, dummy);
        num S0 = (real)0.0; real A0 = (real)0.0;
        for (int i = 0; i < N; ++i) {
            const num* v = V + (size_t)i * D; num quad = (real)0.0;
            for (int r = 0; r < D; ++r) { num t = (real)0.0; for (int q = 0; q < D; ++q) t += Bm[r * D + q] * v[q]; quad += v[r] * t; }
            const num l = N_EXP((real)-0.5 * quad);
            S0 += FN(cb)(c, a, i) * l; A0 += R_ABS(FN(cb)(c, a, i)) * E_ABS(l);
#ifndef CPLX
            if (Lout) Lout[(size_t)a * N + i] = sf2 / N_SQRT(detm) * l;
#endif
        }
        mu[a] = sf2 / N_SQRT(detm) * S0;
        if (Amn) Amn[a] = N_ABS(sf2 / N_SQRT(detm)) * A0;
        for (int r = 0; r < D; ++r) for (int q = 0; q < D; ++q) { Mx[r * D + q] = S[r * D + q] + (r == q ? (real)0.5 * (real)la[r] : (real)0.0); tmp[r * D + q] = (real)2.0 * S[r * D + q] / (real)la[r] + (r == q ? (real)1.0 : (real)0.0); }
        FN(inv_det)(D, Mx, Am);
        const num det2 = FN(inv_det)(D, tmp, dummy);
        for (int i = 0; i < N; ++i) {
            const num* v = V + (size_t)i * D; num g = (real)0.0;
            for (int r = 0; r < D; ++r) { num t = (real)0.0; for (int q = 0; q < D; ++q) t += Am[r * D + q] * v[q]; AV[(size_t)i * D + r] = t; g += v[r] * t; }
            gq[i] = g;
        }
#pragma omp parallel for schedule(dynamic, 8)
        for (int i = 0; i < N; ++i) {
            const num* avi = AV + (size_t)i * D; num row = (real)0.0; real ra = (real)0.0;
            for (int j = i; j < N; ++j) {
                const num* vj = V + (size_t)j * D; num G = (real)0.0;
                for (int r = 0; r < D; ++r) G += vj[r] * avi[r];
                const num E = N_EXP((real)-0.125 * (gq[i] + (real)2.0 * G + gq[j])); const real w = FN(cm)(c, a, i, j);
                row += w * E; ra += R_ABS(w) * E_ABS(E);
            }
            rowz[i] = row; rowa[i] = ra;
        }
        num T = (real)0.0; real AT = (real)0.0;
        for (int i = 0; i < N; ++i) { T += rowz[i]; AT += rowa[i]; }
        const num cv = (real)1.0 / N_SQRT(det2);
        mt[a] = mu[a];
        ct[a * ds + a] = sf2 - cv * T - mu[a] * mu[a];
        if (Ac) Ac[a * ds + a] = sf2 + N_ABS(cv) * AT + N_ABS(mu[a]) * N_ABS(mu[a]);
    }
    /* cross-covariances, consistent form (src/tools/uncertainty_prop.py:187-237; :402-465 with z1^T A z2) */
    for (int a = 0; a < ds; ++a)
        for (int b = bug ? 0 : a + 1; b < ds; ++b) {
            if (b == a) continue;
            const double* la = c->lam + a * D; const double* lb = c->lam + b * D;
            num Rm[MAXD * MAXD], Ri[MAXD * MAXD], Am[MAXD * MAXD];
            for (int r = 0; r < D; ++r) for (int q = 0; q < D; ++q) Rm[r * D + q] = S[r * D + q] * ((real)1.0 / (real)la[q] + (real)1.0 / (real)lb[q]) + (r == q ? (real)1.0 : (real)0.0);
            const num detR = FN(inv_det)(D, Rm, Ri);
            for (int r = 0; r < D; ++r) for (int q = 0; q < D; ++q) { num t = (real)0.0; for (int l = 0; l < D; ++l) t += Ri[r * D + l] * S[l * D + q]; Am[r * D + q] = t; }
            for (int i = 0; i < N; ++i) {
                const num* v = V + (size_t)i * D; num z1[MAXD], z2[MAXD], k1 = (real)0.0, k2 = (real)0.0, q1 = (real)0.0, q2 = (real)0.0;
                for (int r = 0; r < D; ++r) { z1[r] = -v[r] / (real)la[r]; z2[r] = -v[r] / (real)lb[r]; k1 += v[r] * v[r] / (real)la[r]; k2 += v[r] * v[r] / (real)lb[r]; }
                const num* zc = bug ? z2 : z1;     /* the row side of the cross term */
                for (int q = 0; q < D; ++q) { num t = (real)0.0; for (int r = 0; r < D; ++r) t += zc[r] * Am[r * D + q]; AV[(size_t)i * D + q] = t; }
                for (int r = 0; r < D; ++r) { num s1 = (real)0.0, s2 = (real)0.0; for (int q = 0; q < D; ++q) { s1 += Am[r * D + q] * z1[q]; s2 += Am[r * D + q] * z2[q]; } q1 += z1[r] * s1; q2 += z2[r] * s2; Z2[(size_t)i * D + r] = bug ? z1[r] : z2[r]; }
                gq[2 * i] = (real)-0.5 * k1 + (real)0.5 * q1; gq[2 * i + 1] = (real)-0.5 * k2 + (real)0.5 * q2;
            }
#pragma omp parallel for schedule(static)
            for (int i = 0; i < N; ++i) {
                const num* wi = AV + (size_t)i * D; num row = (real)0.0; real ra = (real)0.0;
                for (int j = 0; j < N; ++j) {
                    const num* zj = Z2 + (size_t)j * D; num cr = (real)0.0;
                    for (int r = 0; r < D; ++r) cr += wi[r] * zj[r];
                    const num E = N_EXP(gq[2 * i] + gq[2 * j + 1] + cr); const real w = FN(cb)(c, b, j);
                    row += w * E; ra += R_ABS(w) * E_ABS(E);
                }
                rowz[i] = FN(cb)(c, a, i) * row; rowa[i] = R_ABS(FN(cb)(c, a, i)) * ra;
            }
            num Qs = (real)0.0; real AQ = (real)0.0;
            for (int i = 0; i < N; ++i) { Qs += rowz[i]; AQ += rowa[i]; }
            const real sfab = (real)c->sf[a] * (real)c->sf[a] * (real)c->sf[b] * (real)c->sf[b];
            const num cab = sfab / N_SQRT(detR);
            const num cov = cab * Qs - mu[a] * mu[b];
            ct[a * ds + b] = cov; if (!bug) ct[b * ds + a] = cov;
            if (Ac) { const real A = N_ABS(cab) * AQ + N_ABS(mu[a]) * N_ABS(mu[b]); Ac[a * ds + b] = A; if (!bug) Ac[b * ds + a] = A; }
        }
}

/* One trajectory: means [H+1][ds], covs [H+1][ds][ds] (diagonal rollout: off-diagonal zeros); returns the cost of
 * src/mpc.py:179-198.  Start and action noise as src/dynamics.py:145-163: Sigma_0 = 1e-3 I, action variance float32(1e-3), unless the
 * noise model of the pack is given: init_cov [ds][ds] (the diagonal rollout takes its diagonal), action_var [da], process_var [ds] added
 * to the predicted variance of every step t >= 1.  NULL keeps the constants and the bits. */
static num FN(rollout_one)(const ctx_t* c, int full, const double* x0, const num* U, num* means, num* covs) {
    const int N = c->N, ds = c->ds, da = c->da, D = c->D, H = c->H;
    for (int k = 0; k < ds; ++k) {
        means[k] = (real)x0[k];
        for (int l = 0; l < ds; ++l) {
            if (!c->init_cov) covs[k * ds + l] = (k == l) ? (real)1e-3 : (real)0.0;
            else covs[k * ds + l] = (full || k == l) ? (real)c->init_cov[k * ds + l] : (real)0.0;
        }
    }
    num* V = (num*)malloc(sizeof(num) * (size_t)N * D);
    num* AV = (num*)malloc(sizeof(num) * (size_t)N * D);
    num* gq = (num*)malloc(sizeof(num) * (size_t)N * 2);
    num* Z2 = (num*)malloc(sizeof(num) * (size_t)N * D);
    num* rowz = (num*)malloc(sizeof(num) * (size_t)N);
    real* rowa = (real*)malloc(sizeof(real) * (size_t)N * 2);
    const real act_var = (real)(double)1e-3f;
    for (int t = 1; t <= H; ++t) {
        num u[MAXD], S[MAXD * MAXD], s[MAXD], vt[MAXD];
        num* ct = covs + (size_t)t * ds * ds;
        for (int k = 0; k < D * D; ++k) S[k] = (real)0.0;
        for (int k = 0; k < ds; ++k) { u[k] = means[(t - 1) * ds + k]; for (int l = 0; l < ds; ++l) S[k * D + l] = covs[((size_t)(t - 1) * ds + k) * ds + l]; }
        for (int k = 0; k < da; ++k) { u[ds + k] = U[(t - 1) * da + k]; S[(ds + k) * D + ds + k] = c->action_var ? (real)c->action_var[k] : act_var; }
        if (full) FN(step_full)(c, u, S, 0, means + (size_t)t * ds, ct, 0, 0, 0, V, AV, gq, Z2, rowz, rowa);
        else {
            for (int k = 0; k < D; ++k) s[k] = S[k * D + k];
            FN(step_diag)(c, u, s, means + (size_t)t * ds, vt, 0, 0, 0, rowz, rowa, rowa + N);
            for (int k = 0; k < ds; ++k) for (int l = 0; l < ds; ++l) ct[k * ds + l] = (k == l) ? vt[k] : (num)(real)0.0;
        }
        if (c->process_var) for (int k = 0; k < ds; ++k) ct[k * ds + k] += (real)c->process_var[k];
    }
    free(V); free(AV); free(gq); free(Z2); free(rowz); free(rowa);
    num total = (real)0.0;
    const real g = (real)c->gamma;
    for (int i = 0; i <= H; ++i) {
        const num* m = means + (size_t)i * ds; const num* Sg = covs + (size_t)i * ds * ds;
        num a[MAXD * 2 * MAXD], e[MAXD];
        for (int k = 0; k < ds; ++k) e[k] = m[k] - (real)c->xref[k];
        if (g == (real)0.0) {
            for (int r = 0; r < ds; ++r) { num qe = (real)0.0; for (int q = 0; q < ds; ++q) { qe += (real)c->Q[r * ds + q] * e[q]; total += (real)c->Q[r * ds + q] * Sg[q * ds + r]; } total += e[r] * qe; }
            continue;
        }
        for (int r = 0; r < ds; ++r) for (int q = 0; q < ds; ++q) {
            num t = (real)0.0; for (int l = 0; l < ds; ++l) t += (real)c->Q[r * ds + l] * Sg[l * ds + q];
            a[r * 2 * ds + q] = (r == q ? (real)1.0 : (real)0.0) + g * t; a[r * 2 * ds + ds + q] = (real)c->Q[r * ds + q];
        }
        const num det = FN(gauss_jordan)(ds, ds, a, 2 * ds);          /* (Q^-1 + g Sig)^-1 = (I + g Q Sig)^-1 Q */
        num quad = (real)0.0;
        for (int r = 0; r < ds; ++r) { num t = (real)0.0; for (int q = 0; q < ds; ++q) t += a[r * 2 * ds + ds + q] * e[q]; quad += e[r] * t; }
        total += N_LOG(det) / g + quad;
    }
    for (int j = 0; j < H; ++j)
        for (int k = 0; k < da; ++k) { num rd = (real)0.0; for (int l = 0; l < da; ++l) rd += (real)c->R[k * da + l] * (U[j * da + l] - (real)c->uref[l]); total += (U[j * da + k] - (real)c->uref[k]) * rd; }
    return total;
}

static int FN(bad_shape)(int N, int Np, int ds, int D) { return D > MAXD || ds < 1 || ds > D || N < 1 || Np < N; }

/* B trajectories.  Real builds: means [B][H+1][ds], covs [B][H+1][ds] (full = 0) or [B][H+1][ds][ds] (full = 1), cost [B];
 * grad is not touched.  Complex builds: cost [B] and grad [B][H][da] by the complex step, one run per entry of U
 * (h = 1e-20: no subtraction, exact to rounding); means / covs are not touched. */
int FN(gpmpc_given_rollout)(int full, int N, int Np, int ds, int da, int H, int B, const double* X, const double* lam,
                            const double* sf, const void* beta, const void* M, int cld, const double* x0, const double* U,
                            double gamma, const double* Q, const double* R, const double* xref, const double* uref,
                            double* means, double* covs, double* cost, double* grad, int nthreads,
                            const double* init_cov, const double* action_var, const double* process_var) {
    const int D = ds + da, n = H * da;
    if (FN(bad_shape)(N, Np, ds, D) || H < 1) return -1;
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
    const ctx_t c = {N, Np, ds, da, D, H, X, lam, sf, beta, M, cld, gamma, Q, R, xref, uref, init_cov, action_var, process_var};
    num* Uc = (num*)malloc(sizeof(num) * (size_t)n);
    num* m = (num*)malloc(sizeof(num) * (size_t)(H + 1) * ds);
    num* s = (num*)malloc(sizeof(num) * (size_t)(H + 1) * ds * ds);
    if (!Uc || !m || !s) { free(Uc); free(m); free(s); return -2; }
    for (int b = 0; b < B; ++b) {
        const double* Ub = U + (size_t)b * n;
#ifdef CPLX
        const real h = (real)1e-20;
        for (int e = 0; e < n; ++e) {
            for (int k = 0; k < n; ++k) Uc[k] = (real)Ub[k] + (k == e ? h : (real)0.0) * I;
            const num v = FN(rollout_one)(&c, full, x0 + (size_t)b * ds, Uc, m, s);
            grad[(size_t)b * n + e] = (double)(__imag__ v / h);
            if (e == 0) cost[b] = (double)(__real__ v);
        }
        (void)means; (void)covs;
#else
        for (int k = 0; k < n; ++k) Uc[k] = (real)Ub[k];
        cost[b] = (double)FN(rollout_one)(&c, full, x0 + (size_t)b * ds, Uc, m, s);
        for (int t = 0; t <= H; ++t) for (int k = 0; k < ds; ++k) {
            means[((size_t)b * (H + 1) + t) * ds + k] = (double)m[t * ds + k];
            if (full) for (int l = 0; l < ds; ++l) covs[(((size_t)b * (H + 1) + t) * ds + k) * ds + l] = (double)s[((size_t)t * ds + k) * ds + l];
            else covs[((size_t)b * (H + 1) + t) * ds + k] = (double)s[((size_t)t * ds + k) * ds + k];
        }
        (void)grad;
#endif
    }
    free(Uc); free(m); free(s);
    return 0;
}

#ifndef CPLX
/* nq diagonal steps: u, s [nq][D] -> mean, var, Amean, Avar, Aexp [nq][ds] */
int FN(gpmpc_given_step_diag)(int N, int Np, int ds, int D, const double* X, const double* lam, const double* sf,
                              const void* beta, const void* M, int cld, int nq, const double* u, const double* s,
                              double* mean, double* var, double* Amean, double* Avar, double* Aexp, int nthreads) {
    if (FN(bad_shape)(N, Np, ds, D)) return -1;
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
    const ctx_t c = {N, Np, ds, D - ds, D, 1, X, lam, sf, beta, M, cld, 0.0, 0, 0, 0, 0};
    num* rowz = (num*)malloc(sizeof(num) * (size_t)N);
    real* rowa = (real*)malloc(sizeof(real) * (size_t)N * 2);
    if (!rowz || !rowa) { free(rowz); free(rowa); return -2; }
    for (int q = 0; q < nq; ++q) {
        num uu[MAXD], ss[MAXD], mt[MAXD], vt[MAXD]; real Am[MAXD], Av[MAXD], Ax[MAXD];
        for (int k = 0; k < D; ++k) { uu[k] = (real)u[(size_t)q * D + k]; ss[k] = (real)s[(size_t)q * D + k]; }
        FN(step_diag)(&c, uu, ss, mt, vt, Am, Av, Ax, rowz, rowa, rowa + N);
        for (int a = 0; a < ds; ++a) {
            mean[(size_t)q * ds + a] = (double)mt[a]; var[(size_t)q * ds + a] = (double)vt[a];
            Amean[(size_t)q * ds + a] = (double)Am[a]; Avar[(size_t)q * ds + a] = (double)Av[a]; Aexp[(size_t)q * ds + a] = (double)Ax[a];
        }
    }
    free(rowz); free(rowa);
    return 0;
}

/* nq full-covariance steps: u [nq][D], S [nq][D][D] -> mean and Amean [nq][ds], cov and Acov [nq][ds][ds]; bug: see step_full;
 * lout [nq][ds][N] or NULL: the vector l of every GP, rounded to double. */
int FN(gpmpc_given_step_full)(int N, int Np, int ds, int D, const double* X, const double* lam, const double* sf,
                              const void* beta, const void* M, int cld, int nq, const double* u, const double* S,
                              double* mean, double* cov, double* Amean, double* Acov, int nthreads, int bug, double* lout) {
    if (FN(bad_shape)(N, Np, ds, D)) return -1;
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
    const ctx_t c = {N, Np, ds, D - ds, D, 1, X, lam, sf, beta, M, cld, 0.0, 0, 0, 0, 0};
    num* scr = (num*)malloc(sizeof(num) * (size_t)N * (3 * D + 3));
    real* rowa = (real*)malloc(sizeof(real) * (size_t)N);
    real* lbuf = lout ? (real*)malloc(sizeof(real) * (size_t)ds * N) : 0;
    if (!scr || !rowa || (lout && !lbuf)) { free(scr); free(rowa); free(lbuf); return -2; }
    const size_t nd = (size_t)N * D;
    for (int q = 0; q < nq; ++q) {
        num uu[MAXD], SS[MAXD * MAXD], mt[MAXD], ct[MAXD * MAXD]; real Am[MAXD], Ac[MAXD * MAXD];
        for (int k = 0; k < D; ++k) uu[k] = (real)u[(size_t)q * D + k];
        for (int k = 0; k < D * D; ++k) SS[k] = (real)S[(size_t)q * D * D + k];
        FN(step_full)(&c, uu, SS, bug, mt, ct, Am, Ac, lbuf, scr, scr + nd, scr + 2 * nd, scr + 2 * nd + 2 * (size_t)N, scr + 3 * nd + 2 * (size_t)N, rowa);
        if (lout) for (size_t k = 0; k < (size_t)ds * N; ++k) lout[(size_t)q * ds * N + k] = (double)lbuf[k];
        for (int a = 0; a < ds; ++a) {
            mean[(size_t)q * ds + a] = (double)mt[a]; Amean[(size_t)q * ds + a] = (double)Am[a];
            for (int b = 0; b < ds; ++b) { cov[((size_t)q * ds + a) * ds + b] = (double)ct[a * ds + b]; Acov[((size_t)q * ds + a) * ds + b] = (double)Ac[a * ds + b]; }
        }
    }
    free(scr); free(rowa); free(lbuf);
    return 0;
}
#endif

#ifdef CPLX
/* Jacobians of nq full-covariance steps by the complex step (h = 1e-20: no subtraction, exact to rounding), at sym(S) = (S + S^T)/2:
 *   dmean_du [nq][ds][D], dmean_dS [nq][ds][D][D], dcov_du [nq][ds][ds][D], dcov_dS [nq][ds][ds][D][D];
 * one run per u_k, and one per pair k <= l along the SYMMETRIC direction (E_kl + E_lk)/2, written to [k][l] and [l][k]: the
 * symmetrised derivative include/gpmpc.h promises and sym(autograd) gives.  The diagonal (a, a) of dcov is the variance Jacobian.
 * bug: see step_full (both [a][b] and [b][a] are then derivatives of sums of their own). */
int FN(gpmpc_given_step_full_jac)(int N, int Np, int ds, int D, const double* X, const double* lam, const double* sf,
                                  const void* beta, const void* M, int cld, int nq, const double* u, const double* S, int bug,
                                  double* dmean_du, double* dmean_dS, double* dcov_du, double* dcov_dS, int nthreads) {
    if (FN(bad_shape)(N, Np, ds, D)) return -1;
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
    const ctx_t c = {N, Np, ds, D - ds, D, 1, X, lam, sf, beta, M, cld, 0.0, 0, 0, 0, 0};
    num* scr = (num*)malloc(sizeof(num) * (size_t)N * (3 * D + 3));
    real* rowa = (real*)malloc(sizeof(real) * (size_t)N);
    if (!scr || !rowa) { free(scr); free(rowa); return -2; }
    const size_t nd = (size_t)N * D;
    const real h = (real)1e-20;
    for (int q = 0; q < nq; ++q) {
        num uu[MAXD], SS[MAXD * MAXD], mt[MAXD], ct[MAXD * MAXD];
        for (int k = 0; k < D; ++k) {
                for (int m = 0; m < D; ++m) uu[m] = (real)u[(size_t)q * D + m] + (m == k ? h : (real)0.0) * I;
                for (int r = 0; r < D; ++r) for (int m = 0; m < D; ++m) SS[r * D + m] = (real)0.5 * ((real)S[((size_t)q * D + r) * D + m] + (real)S[((size_t)q * D + m) * D + r]);
                FN(step_full)(&c, uu, SS, bug, mt, ct, 0, 0, 0, scr, scr + nd, scr + 2 * nd, scr + 2 * nd + 2 * (size_t)N, scr + 3 * nd + 2 * (size_t)N, rowa);
                for (int a = 0; a < ds; ++a) {
                    dmean_du[((size_t)q * ds + a) * D + k] = (double)(__imag__ mt[a] / h);
                    for (int b = 0; b < ds; ++b) dcov_du[(((size_t)q * ds + a) * ds + b) * D + k] = (double)(__imag__ ct[a * ds + b] / h);
                }
        }
        for (int k = 0; k < D; ++k)
            for (int l = k; l < D; ++l) {
                for (int m = 0; m < D; ++m) uu[m] = (real)u[(size_t)q * D + m];
                for (int r = 0; r < D; ++r) for (int m = 0; m < D; ++m) SS[r * D + m] = (real)0.5 * ((real)S[((size_t)q * D + r) * D + m] + (real)S[((size_t)q * D + m) * D + r]);
                if (k == l) SS[k * D + k] += h * I;
                else { SS[k * D + l] += (real)0.5 * h * I; SS[l * D + k] += (real)0.5 * h * I; }
                FN(step_full)(&c, uu, SS, bug, mt, ct, 0, 0, 0, scr, scr + nd, scr + 2 * nd, scr + 2 * nd + 2 * (size_t)N, scr + 3 * nd + 2 * (size_t)N, rowa);
                for (int a = 0; a < ds; ++a) {
                    const double dm = (double)(__imag__ mt[a] / h);
                    dmean_dS[(((size_t)q * ds + a) * D + k) * D + l] = dm; dmean_dS[(((size_t)q * ds + a) * D + l) * D + k] = dm;
                    for (int b = 0; b < ds; ++b) {
                        const double dc = (double)(__imag__ ct[a * ds + b] / h);
                        dcov_dS[((((size_t)q * ds + a) * ds + b) * D + k) * D + l] = dc; dcov_dS[((((size_t)q * ds + a) * ds + b) * D + l) * D + k] = dc;
                    }
                }
            }
    }
    free(scr); free(rowa);
    return 0;
}
#endif

#if defined(LDBL) && !defined(CPLX)
/* beta [ds][N] and M [ds][N][N] ((i <= j) at [j][i], off-diagonal pairs doubled, the rest zero) in long double from
 * Ky_inv: gpmpc_cpu_ld.c:30-42, operation by operation (the doubling is exact). */
int gpmpc_given_constants_ld(int N, int ds, int D, const double* X, const double* Kinv, const double* Y, const double* lam,
                             const double* sf, long double* beta, long double* M) {
    if (bad_shape_ld(N, N, ds, D)) return -1;
    for (int a = 0; a < ds; ++a) {
        const double* K = Kinv + (size_t)a * N * N;
#pragma omp parallel for
        for (int i = 0; i < N; ++i) { real t = 0.0L; for (int j = 0; j < N; ++j) t += (real)K[(size_t)i * N + j] * (real)Y[(size_t)j * ds + a]; beta[(size_t)a * N + i] = t; }
        const real sf2 = (real)sf[a] * (real)sf[a], sf4 = sf2 * sf2;
#pragma omp parallel for
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) {
                real w = 0.0L;
                if (i <= j) {
                    real d2 = 0.0L;
                    for (int k = 0; k < D; ++k) { const real d = (real)X[(size_t)i * D + k] - (real)X[(size_t)j * D + k]; d2 += d * d / (real)lam[a * D + k]; }
                    w = (i == j ? 1.0L : 2.0L) * ((0.5L * ((real)K[(size_t)i * N + j] + (real)K[(size_t)j * N + i]) - beta[(size_t)a * N + i] * beta[(size_t)a * N + j]) * sf4 * expl(-0.25L * d2));
                }
                M[((size_t)a * N + j) * N + i] = w;
            }
    }
    return 0;
}
#endif
