// Linearised propagation with the FULL covariance and a linear state feedback u = v + K (x - mu): Sigma' = diag(s2) + G Sigma_z G^T with
// Sigma_z = T Sigma T^T + diag(0, action_var), T = [I; K], and the step Jacobian over the packed state s = (mu, Sigma_kl for k <= l).
// Formulas, layouts and refusals: include/gpmpc.h, "Linearised propagation, full covariance"; the why: DESIGN.md section 3k.
//
// Stage A is the diagonal step itself (linprop.hip's dispatcher, TILE or STREAM as selected), run on a copy of the model's tail with
// action_var = 0 and on a zeroed var_prev, with the Jacobian: its outputs are then m, s2 = sf^2 - q + process_var, g (the mu' rows) and
// -dq/dz (the v' rows: h is an exact zero).  All the O(N^2) work is there.  What this file adds:
//   k_lpf_hess   per (column, GP, 64-row block): the D (D + 1) / 2 sums  sum_i beta_i k_i d_id d_il  (d <= l) and sum_i beta_i k_i; k is
//                recomputed from X (N exp per (column, GP)).  Threads as k_lp_hess: (c = t & 63, q = t >> 6) owns column c and 16 rows.
//   k_lpf_hfin   row blocks added in ascending order, [d = l] / lambda subtracted -> Hm[column][GP][d <= l]
//   k_lpf_close  one wave per column: Sigma_z, P = G T, W_b = Sigma_z G_b^T, then Sigma' (a <= b, mirrored) and the packed Jacobian, every
//                element written.  Each element is owned by one lane, which sums in ascending index order.
//   k_lpf_init   step 0 of a rollout: mu_0 = x0, Sigma_0 = init_cov
//   k_lpf_vjp    the adjoint sweep over the packed Jacobians, one wave per plan, lane c owns column c (the layout of k_rollout_vjp)
//   k_lpf_constraints   the forward-sensitivity sweep of the chance constraints, one lane per column of the dense Jacobian
// Rules: no atomics; launch geometry from the sizes only; columns are independent, so nothing depends on `chunk`; two identical calls
// agree bit for bit; the rollout is the chain of step calls.
#include <cmath>
#include "linprop_internal.h"                   // the model frame, LpTail, LpHyp, LpIn, and the dispatcher of linprop.hip

#define LPF_T GPMPC_MODEL_TILE                  // columns / rows per tile: what the chunk rule of model_frame.h rounds to
#define LPF_MAX_TRI (GPMPC_MAX_DS * (GPMPC_MAX_DS + 1) / 2)
#define LPF_MAX_P (GPMPC_MAX_DS + LPF_MAX_TRI)

struct LpfNoise { double init_cov[GPMPC_MAX_DS * GPMPC_MAX_DS]; double action_var[GPMPC_MAX_D]; };

// index e of the row-major upper triangle of an n x n matrix -> (a, b), a <= b; and back
static __host__ __device__ __forceinline__ void lpf_untri(int e, int n, int& a, int& b) {
    a = 0;
    while (e >= n - a) { e -= n - a; ++a; }
    b = a + e;
}
static __host__ __device__ __forceinline__ int lpf_tri(int a, int b, int n) { return a * n - a * (a - 1) / 2 + (b - a); }

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// grid (cnp / 64, ceil(n / 64), ds).  hpart[bi][a][v][c], v < NH = D (D + 1) / 2: the (d <= l) sums, row-major; v = NH: sum_i beta_i k_i.
template <int D>
__global__ __launch_bounds__(256) void k_lpf_hess(int n, int cn, int ds, const double* __restrict__ X, LpIn I, const double* __restrict__ beta,
                                                   LpHyp Hy, double* __restrict__ hpart, int ldk) {
    constexpr int NH = D * (D + 1) / 2;
    __shared__ double s_x[LPF_T][D], s_b[LPF_T], s_p[3][NH + 1][LPF_T];
    const int t = threadIdx.x, c = t & 63, q = t >> 6, a = blockIdx.z;
    const int c0 = blockIdx.x * LPF_T, i0 = blockIdx.y * LPF_T;
    for (int e = t; e < LPF_T * D; e += 256) {
        const int i = e / D, d = e - i * D;
        s_x[i][d] = i0 + i < n ? X[(size_t)(i0 + i) * D + d] : 0.0;
    }
    if (t < LPF_T) s_b[t] = i0 + t < n ? beta[(size_t)(i0 + t) * ds + a] : 0.0;
    const bool live = c0 + c < cn;
    double z[D], il[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        z[d] = live ? lp_z(I, c0 + c, d, ds) : 0.0;
        il[d] = Hy.ilam[a][d];
    }
    const double sf2 = Hy.sf2[a];
    __syncthreads();
    double acc[NH + 1];
#pragma unroll
    for (int v = 0; v <= NH; ++v) acc[v] = 0.0;
    for (int r = 0; r < 16; ++r) {
        const int row = 16 * q + r;
        double d2 = 0.0, dd[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double u = s_x[row][d] - z[d];
            d2 = fma(u * u, il[d], d2);
            dd[d] = u * il[d];
        }
        const double k = (i0 + row < n && live) ? sf2 * exp(-0.5 * d2) : 0.0;
        const double bk = s_b[row] * k;
        acc[NH] = acc[NH] + bk;
        int v = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double bd = bk * dd[d];
#pragma unroll
            for (int l = d; l < D; ++l, ++v) acc[v] = fma(bd, dd[l], acc[v]);
        }
    }
    if (q > 0) {
#pragma unroll
        for (int v = 0; v <= NH; ++v) s_p[q - 1][v][c] = acc[v];
    }
    __syncthreads();
    if (q == 0) {
        double* __restrict__ out = hpart + ((size_t)blockIdx.y * ds + a) * (NH + 1) * ldk + c0 + c;
#pragma unroll
        for (int v = 0; v <= NH; ++v) out[(size_t)v * ldk] = (acc[v] + s_p[0][v][c]) + (s_p[1][v][c] + s_p[2][v][c]);
    }
}

// one thread per (GP, v < NH, column): Hm[c][a][v] = sum over the row blocks, ascending, - [d = l] (sum_i beta_i k_i) / lambda_ad
__global__ __launch_bounds__(256) void k_lpf_hfin(int cn, int nbi, int D, int ds, LpHyp Hy, const double* __restrict__ hpart, int ldk,
                                                   double* __restrict__ Hm) {
    const int NH = D * (D + 1) / 2;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)cn * ds * NH) return;
    const int c = (int)(e % cn), av = (int)(e / cn), a = av / NH, v = av - a * NH;
    double s = 0.0;
    for (int b = 0; b < nbi; ++b) s += hpart[(((size_t)b * ds + a) * (NH + 1) + v) * ldk + c];
    int d, l;
    lpf_untri(v, D, d, l);
    if (d == l) {
        double s0 = 0.0;
        for (int b = 0; b < nbi; ++b) s0 += hpart[(((size_t)b * ds + a) * (NH + 1) + NH) * ldk + c];
        s = s - s0 * Hy.ilam[a][d];
    }
    Hm[((size_t)c * ds + a) * NH + v] = s;
}

// grid (B), one wave per column.  a_var = s2, column b at + b vs; a_jac [B][2ds][2ds+da] = stage A's Jacobian (rows mu': g; rows v': -dq/dz),
// Hm [B][ds][NH] (JAC only).  cov_prev: the column's matrix at + b cs (upper triangle read); K [da][ds] or null.
template <bool JAC>
__global__ __launch_bounds__(64) void k_lpf_close(int ds, int da, LpfNoise N, const double* __restrict__ cov_prev, size_t cs,
                                                  const double* __restrict__ K, const double* __restrict__ a_var, size_t vs,
                                                  const double* __restrict__ a_jac, const double* __restrict__ Hm,
                                                  double* __restrict__ out_cov, size_t ocs, double* __restrict__ jac, size_t js) {
    constexpr int M = GPMPC_MAX_D;
    __shared__ double S[M][M], Kg[M][M], G[M][M], mdq[M][M], KS[M][M], Sz[M][M], P[M][M], W[M][M], s2[M];
    __shared__ double Hs[JAC ? GPMPC_MAX_DS : 1][JAC ? M : 1][JAC ? M : 1];
    __shared__ int tab[LPF_MAX_TRI][2];
    const int b = blockIdx.x, t = threadIdx.x, D = ds + da, ncA = 2 * ds + da, nt = ds * (ds + 1) / 2, p = ds + nt, nc = p + da;
    const double* __restrict__ Cp = cov_prev + (size_t)b * cs;
    const double* __restrict__ Ja = a_jac + (size_t)b * (2 * ds) * ncA;
    for (int e = t; e < ds * ds; e += 64) {
        const int k = e / ds, l = e - k * ds;
        S[k][l] = Cp[k <= l ? k * ds + l : l * ds + k];
    }
    for (int e = t; e < da * ds; e += 64) {
        const int j = e / ds, k = e - j * ds;
        Kg[j][k] = K ? K[e] : 0.0;
    }
    for (int e = t; e < ds * D; e += 64) {
        const int a = e / D, d = e - a * D, col = d < ds ? d : ds + d;
        G[a][d] = Ja[a * ncA + col];
        mdq[a][d] = Ja[(ds + a) * ncA + col];
    }
    if (t < ds) s2[t] = a_var[(size_t)b * vs + t];
    if (t < nt) {
        int a, bb;
        lpf_untri(t, ds, a, bb);
        tab[t][0] = a; tab[t][1] = bb;
    }
    if (JAC) {
        const int NH = D * (D + 1) / 2;
        for (int e = t; e < ds * NH; e += 64) {
            const int a = e / NH, v = e - a * NH;
            int d, l;
            lpf_untri(v, D, d, l);
            const double h = Hm[((size_t)b * ds + a) * NH + v];
            Hs[JAC ? a : 0][JAC ? d : 0][JAC ? l : 0] = h;
            Hs[JAC ? a : 0][JAC ? l : 0][JAC ? d : 0] = h;
        }
    }
    __syncthreads();
    // K Sigma, and the closed-loop gradient P = G T
    for (int e = t; e < da * ds; e += 64) {
        const int j = e / ds, k = e - j * ds;
        double s = 0.0;
        for (int m = 0; m < ds; ++m) s = fma(Kg[j][m], S[m][k], s);
        KS[j][k] = s;
    }
    for (int e = t; e < ds * ds; e += 64) {
        const int a = e / ds, k = e - a * ds;
        double s = 0.0;
        for (int j = 0; j < da; ++j) s = fma(G[a][ds + j], Kg[j][k], s);
        P[a][k] = G[a][k] + s;
    }
    __syncthreads();
    // Sigma_z = T Sigma T^T + diag(0, action_var): (d <= l) computed, mirrored
    for (int e = t; e < D * D; e += 64) {
        const int d = e / D, l = e - d * D;
        if (d > l) continue;
        double v;
        if (l < ds) v = S[d][l];
        else if (d < ds) v = KS[l - ds][d];
        else {
            const int j = d - ds, i = l - ds;
            double s = 0.0;
            for (int k = 0; k < ds; ++k) s = fma(KS[j][k], Kg[i][k], s);
            v = i == j ? s + N.action_var[j] : s;
        }
        Sz[d][l] = v;
        Sz[l][d] = v;
    }
    __syncthreads();
    for (int e = t; e < ds * D; e += 64) {
        const int a = e / D, d = e - a * D;
        double s = 0.0;
        for (int l = 0; l < D; ++l) s = fma(Sz[d][l], G[a][l], s);
        W[a][d] = s;
    }
    __syncthreads();
    double* __restrict__ Co = out_cov + (size_t)b * ocs;
    if (t < nt) {
        const int a = tab[t][0], bb = tab[t][1];
        double s = 0.0;
        for (int d = 0; d < D; ++d) s = fma(G[a][d], W[bb][d], s);
        if (a == bb) s = s2[a] + s;
        Co[a * ds + bb] = s;
        Co[bb * ds + a] = s;
    }
    if (!JAC) return;
    double* __restrict__ J = jac + (size_t)b * js;
    for (int e = t; e < p * nc; e += 64) {
        const int r = e / nc, c = e - r * nc;
        double v;
        if (r < ds) v = c < ds ? G[r][c] : (c < p ? 0.0 : G[r][ds + (c - p)]);
        else {
            const int a = tab[r - ds][0], bb = tab[r - ds][1];
            if (c >= ds && c < p) {
                const int k = tab[c - ds][0], l = tab[c - ds][1];
                v = k == l ? P[a][k] * P[bb][k] : P[a][k] * P[bb][l] + P[a][l] * P[bb][k];
            } else {
                const int d = c < ds ? c : ds + (c - p);
                double x = 0.0, y = 0.0;
                for (int l = 0; l < D; ++l) x = fma(Hs[JAC ? a : 0][JAC ? d : 0][JAC ? l : 0], W[bb][l], x);
                for (int l = 0; l < D; ++l) y = fma(Hs[JAC ? bb : 0][JAC ? d : 0][JAC ? l : 0], W[a][l], y);
                v = x + y;
                if (a == bb) v = mdq[a][d] + v;
            }
        }
        J[e] = v;
    }
}

// step 0 of a rollout: means[b][0] = x0[b], covs[b][0] = init_cov
__global__ __launch_bounds__(256) void k_lpf_init(int B, int H, int ds, const double* __restrict__ x0, LpfNoise N, double* __restrict__ means,
                                                   double* __restrict__ covs) {
    const int per = ds + ds * ds;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B * per) return;
    const int b = (int)(e / per), r = (int)(e - (long)b * per);
    if (r < ds) means[(size_t)b * (H + 1) * ds + r] = x0[(size_t)b * ds + r];
    else covs[(size_t)b * (H + 1) * ds * ds + (r - ds)] = N.init_cov[r - ds];
}

// grid (B), one wave per plan; lane c owns column c of the packed Jacobians [p][p + da].  add_dU (or null): added to the input columns.
__global__ __launch_bounds__(64) void k_lpf_vjp(int H, int ds, int da, const double* __restrict__ jac, const double* __restrict__ g_means,
                                                const double* __restrict__ g_covs, const double* __restrict__ add_dU,
                                                double* __restrict__ out_gU, double* __restrict__ out_gx0) {
    __shared__ double s_adj[2][LPF_MAX_P];
    const int b = blockIdx.x, c = threadIdx.x, nt = ds * (ds + 1) / 2, p = ds + nt, nc = p + da;
    int ck = 0, cl = 0;
    if (c >= ds && c < p) lpf_untri(c - ds, ds, ck, cl);
    auto seed = [&](int t) {                                 // of this lane's packed variable at step t
        const size_t o = (size_t)b * (H + 1) + t;
        if (c < ds) return g_means ? g_means[o * ds + c] : 0.0;
        if (!g_covs) return 0.0;
        const double* __restrict__ gc = g_covs + o * ds * ds;
        return ck == cl ? gc[ck * ds + ck] : gc[ck * ds + cl] + gc[cl * ds + ck];
    };
    if (c < p) s_adj[0][c] = seed(H);
    __syncthreads();
    int cur = 0;
    for (int t = H; t >= 1; --t) {
        const double* __restrict__ Jt = jac + ((size_t)b * H + (t - 1)) * p * nc;
        if (c < nc) {
            double sum = 0.0;
            for (int r = 0; r < p; ++r) sum = fma(Jt[r * nc + c], s_adj[cur][r], sum);
            if (c < p) s_adj[cur ^ 1][c] = seed(t - 1) + sum;
            else {
                const size_t o = ((size_t)b * H + (t - 1)) * da + (c - p);
                out_gU[o] = add_dU ? add_dU[o] + sum : sum;
            }
        }
        __syncthreads();
        cur ^= 1;
    }
    if (out_gx0 && c < ds) out_gx0[(size_t)b * ds + c] = s_adj[cur][c];      // mu_0 = x0; Sigma_0 is a constant
}

// grid (B, ceil(H da / 64)), one wave per workgroup, lane = column tau da + j of the dense Jacobian.  The column's p sensitivities live in
// LDS, [row][lane]: no lane reads another's.  JAC = false: values only (grid (B, 1)).  The rules of k_rollout_constraints (constraints.hip).
template <int DS, bool JAC>
__global__ __launch_bounds__(64) void k_lpf_constraints(int H, int da, gpmpc_state_constraints C, const double* __restrict__ means,
                                                        const double* __restrict__ covs, const double* __restrict__ jac,
                                                        double* __restrict__ out_g, double* __restrict__ out_gjac) {
    constexpr int NT = DS * (DS + 1) / 2, NP = DS + NT;
    __shared__ double S[JAC ? 2 : 1][JAC ? NP : 1][64];
    const int b = blockIdx.x, lane = threadIdx.x, mc = C.n_rows, nc = NP + da, ncols = H * da;
    const int c0 = blockIdx.y * 64, c = c0 + lane;
    const bool live = c < ncols;
    const int tau = c / da, j = c - tau * da, tau0 = c0 / da;
    const bool first = blockIdx.y == 0;
    int cur = 0;
    if (JAC)
        for (int r = 0; r < NP; ++r) S[0][JAC ? r : 0][lane] = 0.0;
    for (int t = 1; t <= H; ++t) {
        if (JAC && tau0 < t) {
            const double* __restrict__ Jt = jac + ((size_t)b * H + (t - 1)) * NP * nc;
            if (tau0 < t - 1) {
                const bool started = tau < t - 1;
                for (int r = 0; r < NP; ++r) {
                    double acc = 0.0;
                    for (int k = 0; k < NP; ++k) acc = fma(Jt[r * nc + k], S[JAC ? cur : 0][JAC ? k : 0][lane], acc);
                    S[JAC ? cur ^ 1 : 0][JAC ? r : 0][lane] = started ? acc : 0.0;
                }
                cur ^= 1;
            }
            if (live && tau == t - 1)
                for (int r = 0; r < NP; ++r) S[JAC ? cur : 0][JAC ? r : 0][lane] = Jt[r * nc + NP + j];
        }
        const double* __restrict__ mu = means + ((size_t)b * (H + 1) + t) * DS;
        const double* __restrict__ cv = covs + ((size_t)b * (H + 1) + t) * DS * DS;
        for (int r = 0; r < mc; ++r) {
            double am = 0.0, q = 0.0;
            for (int k = 0; k < DS; ++k) {
                const double a = C.A[r * DS + k];
                am = fma(a, mu[k], am);
                for (int l = 0; l < DS; ++l) q = fma(a * C.A[r * DS + l], cv[k * DS + l], q);
            }
            // q <= 0: sd = 0 and no variance part; NaN passes through
            const double sd = q > 0.0 ? sqrt(q) : (q <= 0.0 ? 0.0 : q);
            const double kap = C.kappa[r];
            if (first && lane == 0) out_g[((size_t)b * H + (t - 1)) * mc + r] = fma(kap, sd, am) - C.b[r];
            if (JAC) {
                const double f = q <= 0.0 ? 0.0 : kap / (2.0 * sd);
                double dm = 0.0, dv = 0.0;
                int v = DS;
                for (int k = 0; k < DS; ++k) {
                    const double a = C.A[r * DS + k];
                    dm = fma(a, S[JAC ? cur : 0][JAC ? k : 0][lane], dm);
                    for (int l = k; l < DS; ++l, ++v) {     // the variable Sigma_kl stands for both entries (k, l) and (l, k)
                        const double w = k == l ? a * a : 2.0 * (a * C.A[r * DS + l]);
                        dv = fma(w, S[JAC ? cur : 0][JAC ? v : 0][lane], dv);
                    }
                }
                if (live) out_gjac[(((size_t)b * H + (t - 1)) * mc + r) * ncols + c] = tau < t ? fma(f, dv, dm) : 0.0;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// host: checks, layouts
// ---------------------------------------------------------------------------
static int lpf_p(int ds) { return ds + ds * (ds + 1) / 2; }
// B H packed Jacobians of at most LPF_MAX_P (LPF_MAX_P + GPMPC_MAX_D) elements stay below 2^40 elements; the constraints sweep runs
// ceil(H da / 64) workgroups per plan in gridDim.y (at most 65535).  The sweeps keep no per-step state: these are the only limits on H.
static bool lpf_count_ok(long B, long H) { return B >= 1 && H >= 1 && B * H * (long)LPF_MAX_P * (LPF_MAX_P + GPMPC_MAX_D) <= (1L << 40); }
static bool lpf_sweep_fits(long H, int da) { return H * (da > 0 ? da : 1) <= 64L * 65535; }

struct LpfModel { LpTail tail, tailA; LpHyp hyp; LpfNoise noise; };
// What the diagonal entries refuse, then the whole init_cov: finite, symmetric (the particles' rule), no negative pivot.
static int lpf_check_model(const char* who, const gpmpc_gp_model* m, LpfModel* out) {
    if (int rc = gpmpc_lp_check_model(who, m, &out->tail)) return rc;
    const int ds = m->state_dim, da = m->action_dim;
    memset(&out->noise, 0, sizeof(out->noise));
    out->hyp = lp_hyp(m);
    for (int a = 0; a < ds; ++a) out->noise.init_cov[a * ds + a] = out->tail.init_var[a];
    for (int j = 0; j < da; ++j) out->noise.action_var[j] = out->tail.action_var[j];
    if (m->has_noise) {
        double big = 0.0;
        for (int k = 0; k < ds * ds; ++k) {
            if (!gpmpc_finite(m->init_cov[k])) return gpmpc_refuse(who, "init_cov holds a non-finite value");
            big = fmax(big, fabs(m->init_cov[k]));
        }
        for (int a = 0; a < ds; ++a)
            for (int b = 0; b < a; ++b)
                if (fabs(m->init_cov[a * ds + b] - m->init_cov[b * ds + a]) > 1e-12 * big) return gpmpc_refuse(who, "init_cov is not symmetric");
        // Cholesky pivots of the upper triangle, mirrored: one below -1e-12 max |P| is a refusal, a zero pivot gives a zero column
        double Pm[GPMPC_MAX_DS * GPMPC_MAX_DS], L[GPMPC_MAX_DS * GPMPC_MAX_DS] = {};
        for (int a = 0; a < ds; ++a)
            for (int b = a; b < ds; ++b) Pm[a * ds + b] = Pm[b * ds + a] = m->init_cov[a * ds + b];
        double d = 0.0;
        int j = 0;
        if (!gpmpc_psd_pivots(Pm, ds, big, L, &d, &j))
            return gpmpc_refuse(who, "init_cov has a negative pivot (%g at %d): it is not positive semi-definite", d, j);
        memcpy(out->noise.init_cov, Pm, sizeof(double) * ds * ds);
    }
    out->tailA = out->tail;
    for (int j = 0; j < GPMPC_MAX_D; ++j) out->tailA.action_var[j] = 0.0;     // stage A: s2 and g only, no input-variance term
    return GPMPC_OK;
}

static int lpf_check_gain(const char* who, const gpmpc_gp_model* m, const double* K, size_t k_step_stride) {
    const size_t full = (size_t)m->action_dim * m->state_dim;
    if (K && m->action_dim == 0) return gpmpc_refuse(who, "a feedback gain needs action_dim >= 1");
    if (k_step_stride != 0 && k_step_stride != full) return gpmpc_refuse(who, "k_step_stride must be 0 or action_dim state_dim");
    return GPMPC_OK;
}

// workspace of a step of B columns whose inputs lie xs doubles apart:
//   zero [(B-1) xs + ds] | s2 [(B-1) xs + ds] | stage A's Jacobian [B][2ds][2ds+da] | with the Jacobian: hpart [nbi][ds][NH+1][C] | Hm [B][ds][NH] | stage A's own
struct LpfLayout { size_t off_zero, zero_bytes, off_var, off_ajac, off_hpart, off_hm, off_a, total; int nbi, C; LpLayout A; };
static LpfLayout lpf_layout(const gpmpc_gp_model* m, long B, size_t xs, bool want_jac, int chunk, gpmpc_carver& c) {
    LpfLayout L;
    const int ds = m->state_dim, da = m->action_dim, D = ds + da, NH = D * (D + 1) / 2;
    const size_t d = sizeof(double);
    L.nbi = (m->n + LPF_T - 1) / LPF_T;
    L.C = gpmpc_chunk_cols(B, chunk);
    L.zero_bytes = d * ((size_t)(B - 1) * xs + ds);
    L.off_zero = c.take(L.zero_bytes);
    L.off_var = c.take(L.zero_bytes);                    // s2 lands with the stride of out_mu: the dispatcher has one output stride
    L.off_ajac = c.take(d * B * (2 * ds) * (2 * ds + da));
    L.off_hpart = c.take(want_jac ? d * L.nbi * ds * (NH + 1) * L.C : 0);
    L.off_hm = c.take(want_jac ? d * B * ds * NH : 0);
    L.A = gpmpc_lp_layout(m, chunk, B, true);
    L.off_a = c.take(L.A.total);
    L.total = c.total();
    return L;
}

// One step.  mu_prev + b xs, cov_prev + b cs, U_t + b us -> out_mu + b os, out_cov + b ocs, jac (or null) + b js.  The zero section of the
// workspace has been cleared by the caller (once per call: every step of a rollout reads the same zeros).
static int lpf_step(const gpmpc_gp_model* m, const LpfModel& M, int B, const double* mu_prev, size_t xs, const double* cov_prev, size_t cs,
                    const double* U_t, size_t us, const double* K_t, double* out_mu, size_t os, double* out_cov, size_t ocs, double* jac, size_t js,
                    const LpfLayout& L, char* ws, hipStream_t s) {
    const int ds = m->state_dim, da = m->action_dim, D = ds + da, NH = D * (D + 1) / 2;
    double* a_var = (double*)(ws + L.off_var);
    double* a_jac = (double*)(ws + L.off_ajac);
    if (int rc = gpmpc_lp_step(m, M.tailA, B, mu_prev, (const double*)(ws + L.off_zero), xs, U_t, us, out_mu, a_var, os, a_jac,
                               (size_t)(2 * ds) * (2 * ds + da), L.A, ws + L.off_a, s))
        return rc;
    if (jac) {
        double* hpart = (double*)(ws + L.off_hpart);
        double* Hm = (double*)(ws + L.off_hm);
        for (long c0 = 0; c0 < B; c0 += L.C) {
            const int cn = (int)(B - c0 < L.C ? B - c0 : L.C), cnp = (cn + LPF_T - 1) / LPF_T * LPF_T;
            LpIn I;
            I.mu = mu_prev + (size_t)c0 * xs; I.var = nullptr; I.U = U_t ? U_t + (size_t)c0 * us : nullptr;
            I.xs = xs; I.us = us;
            if (int rc = gpmpc_dispatch_dim<1>(D, [&](auto dd) {
                    hipLaunchKernelGGL(k_lpf_hess<decltype(dd)::value>, dim3(cnp / LPF_T, L.nbi, ds), dim3(256), 0, s, m->n, cn, ds, m->X, I, m->beta,
                                       M.hyp, hpart, L.C);
                    return GPMPC_OK;
                }))
                return rc;
            hipLaunchKernelGGL(k_lpf_hfin, dim3(gpmpc_blocks256((long)cn * ds * NH)), dim3(256), 0, s, cn, L.nbi, D, ds, M.hyp, (const double*)hpart, L.C,
                               Hm + (size_t)c0 * ds * NH);
        }
        hipLaunchKernelGGL(k_lpf_close<true>, dim3(B), dim3(64), 0, s, ds, da, M.noise, cov_prev, cs, K_t, (const double*)a_var, os,
                           (const double*)a_jac, (const double*)Hm, out_cov, ocs, jac, js);
    } else {
        hipLaunchKernelGGL(k_lpf_close<false>, dim3(B), dim3(64), 0, s, ds, da, M.noise, cov_prev, cs, K_t, (const double*)a_var, os,
                           (const double*)a_jac, (const double*)nullptr, out_cov, ocs, (double*)nullptr, (size_t)0);
    }
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

// ---------------------------------------------------------------------------
// host: entries
// ---------------------------------------------------------------------------
extern "C" size_t gpmpc_linearised_fc_step_workspace_bytes(const gpmpc_gp_model* m, int B, int want_jac, int chunk) {
    if (!gpmpc_model_sizes_ok(m) || !lpf_count_ok(B, 1) || !gpmpc_chunk_ok(chunk)) return 0;
    gpmpc_carver c;
    return lpf_layout(m, B, m->state_dim, want_jac != 0, chunk, c).total;
}

extern "C" int gpmpc_linearised_fc_step(const gpmpc_gp_model* m, int B, const double* mu_prev, const double* cov_prev, const double* U_t,
                                        size_t u_stride, const double* K_dev, double* out_mu, double* out_cov, double* out_jac,
                                        size_t jac_stride, int chunk, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "gpmpc_linearised_fc_step";
    LpfModel M;
    if (int rc = lpf_check_model(who, m, &M)) return rc;
    if (B < 1) return gpmpc_refuse(who, "B < 1");
    if (!lpf_count_ok(B, 1)) return gpmpc_refuse(who, "B is too large");
    if (int rc = gpmpc_check_chunk(who, chunk)) return rc;
    if (!mu_prev || !cov_prev || !out_mu || !out_cov || !workspace || (m->action_dim > 0 && !U_t)) return gpmpc_refuse(who, "NULL pointer");
    if (out_mu == mu_prev || out_cov == cov_prev || out_mu == cov_prev || out_cov == mu_prev || out_mu == out_cov)
        return gpmpc_refuse(who, "the outputs must not alias the inputs or each other");
    if (int rc = lpf_check_gain(who, m, K_dev, 0)) return rc;
    const int ds = m->state_dim, da = m->action_dim, p = lpf_p(ds);
    if (u_stride < (size_t)da && B > 1) return gpmpc_refuse(who, "u_stride < action_dim");
    if (out_jac && jac_stride < (size_t)p * (p + da) && B > 1) return gpmpc_refuse(who, "jac_stride < p (p + da)");
    gpmpc_carver c;
    const LpfLayout L = lpf_layout(m, B, ds, out_jac != nullptr, chunk, c);
    if (workspace_bytes < L.total) return GPMPC_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    GPMPC_HIP(hipMemsetAsync(ws + L.off_zero, 0, L.zero_bytes, s));
    return lpf_step(m, M, B, mu_prev, ds, cov_prev, (size_t)ds * ds, U_t, u_stride, K_dev, out_mu, ds, out_cov, (size_t)ds * ds, out_jac, jac_stride,
                    L, ws, s);
}

extern "C" int gpmpc_linearised_fc_vjp(int B, int H, int ds, int da, const double* jac, const double* g_means, const double* g_covs,
                                       double* out_gU, double* out_gx0, void* stream) {
    const char* who = "gpmpc_linearised_fc_vjp";
    if (!jac || !out_gU) return gpmpc_refuse(who, "NULL pointer");
    if (B < 1 || H < 1) return gpmpc_refuse(who, "B or H < 1");
    if (ds < 1 || ds > GPMPC_MAX_DS || da < 1 || ds + da > GPMPC_MAX_D) return gpmpc_refuse(who, "state_dim or action_dim outside the range");
    if (!lpf_count_ok(B, H)) return gpmpc_refuse(who, "B x H is too large");
    hipLaunchKernelGGL(k_lpf_vjp, dim3(B), dim3(64), 0, (hipStream_t)stream, H, ds, da, jac, g_means, g_covs, (const double*)nullptr, out_gU, out_gx0);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

static int lpf_constraints(int B, int H, int ds, int da, const gpmpc_state_constraints* C, const double* means, const double* covs,
                           const double* jac, double* out_g, double* out_gjac, hipStream_t s) {
    if (int rc = gpmpc_dispatch_dim<1>(ds, [&](auto d) {
            constexpr int DS = decltype(d)::value;
            if (out_gjac)
                hipLaunchKernelGGL((k_lpf_constraints<DS, true>), dim3(B, (H * da + 63) / 64), dim3(64), 0, s, H, da, *C, means, covs, jac, out_g, out_gjac);
            else
                hipLaunchKernelGGL((k_lpf_constraints<DS, false>), dim3(B, 1), dim3(64), 0, s, H, da, *C, means, covs, jac, out_g, out_gjac);
            return GPMPC_OK;
        }))
        return rc;
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

extern "C" int gpmpc_linearised_fc_constraints(int B, int H, int ds, int da, const gpmpc_state_constraints* C, const double* means,
                                               const double* covs, const double* jac, double* out_g, double* out_gjac, void* stream) {
    const char* who = "gpmpc_linearised_fc_constraints";
    if (!C || !means || !covs || !out_g || (out_gjac && !jac)) return gpmpc_refuse(who, "NULL pointer");
    if (B < 1 || H < 1) return gpmpc_refuse(who, "B or H < 1");
    if (ds < 1 || ds > GPMPC_MAX_DS || da < 1 || ds + da > GPMPC_MAX_D) return gpmpc_refuse(who, "state_dim or action_dim outside the range");
    if (!lpf_count_ok(B, H) || !lpf_sweep_fits(H, da)) return gpmpc_refuse(who, "H = %d is beyond the sweep's grid (H da <= 64 x 65535)", H);
    if (int rc = gpmpc_check_constraints(C, who)) return rc;
    return lpf_constraints(B, H, ds, da, C, means, covs, jac, out_g, out_gjac, (hipStream_t)stream);
}

// workspace of a rollout: means [B][H+1][ds] | covs [B][H+1][ds][ds] | with the gradient: jac [B][H][p][p+da], d_means, d_covs, d_U | a step's
struct LpfRollLayout { size_t off_means, off_covs, off_jac, off_dm, off_dc, off_du; LpfLayout step; size_t total; };
static LpfRollLayout lpf_roll_layout(const gpmpc_gp_model* m, int B, int H, bool grad, int chunk) {
    LpfRollLayout R;
    gpmpc_carver c;
    const int ds = m->state_dim, da = m->action_dim, p = lpf_p(ds);
    const size_t d = sizeof(double);
    R.off_means = c.take(d * B * (H + 1) * ds);
    R.off_covs = c.take(d * B * (H + 1) * ds * ds);
    R.off_jac = c.take(grad ? d * B * H * p * (p + da) : 0);
    R.off_dm = c.take(grad ? d * B * (H + 1) * ds : 0);
    R.off_dc = c.take(grad ? d * B * (H + 1) * ds * ds : 0);
    R.off_du = c.take(grad ? d * B * H * da : 0);
    R.step = lpf_layout(m, B, (size_t)(H + 1) * ds, grad, chunk, c);
    R.total = c.total();
    return R;
}

extern "C" size_t gpmpc_linearised_fc_rollout_workspace_bytes(const gpmpc_gp_model* m, int B, int H, unsigned flags, int chunk) {
    if (!gpmpc_model_sizes_ok(m) || !lpf_count_ok(B, H) || !lpf_sweep_fits(H, m->action_dim) || (flags & ~GPMPC_WANT_GRAD) || !gpmpc_chunk_ok(chunk))
        return 0;
    return lpf_roll_layout(m, B, H, (flags & GPMPC_WANT_GRAD) != 0, chunk).total;
}

extern "C" int gpmpc_linearised_fc_rollout(const gpmpc_gp_model* m, int B, int H, const double* x0, const double* U, const double* K_dev,
                                           size_t k_step_stride, const gpmpc_cost_params* cost, const gpmpc_state_constraints* cons,
                                           unsigned flags, double* out_means, double* out_covs, double* out_jac, double* out_cost,
                                           double* out_grad, double* out_g, double* out_gjac, int chunk, void* workspace, size_t workspace_bytes,
                                           void* stream) {
    return gpmpc_lpf_rollout("gpmpc_linearised_fc_rollout", m, B, H, x0, U, K_dev, k_step_stride, cost, cons, flags, out_means, out_covs, out_jac,
                             out_cost, out_grad, out_g, out_gjac, chunk, workspace, workspace_bytes, stream, nullptr);
}

// `in` (or null): the input cost and the input chance constraints of gpmpc_linearised_fc_rollout_inputs (linprop_inputs.hip).  They read the
// trajectory and add to the cost and to the covariance seed of the adjoint sweep: means, covs, jac, g and g_jac never see them.
int gpmpc_lpf_rollout(const char* who, const gpmpc_gp_model* m, int B, int H, const double* x0, const double* U, const double* K_dev,
                      size_t k_step_stride, const gpmpc_cost_params* cost, const gpmpc_state_constraints* cons, unsigned flags, double* out_means,
                      double* out_covs, double* out_jac, double* out_cost, double* out_grad, double* out_g, double* out_gjac, int chunk,
                      void* workspace, size_t workspace_bytes, void* stream, const LpfInputs* in) {
    LpfModel M;
    if (int rc = lpf_check_model(who, m, &M)) return rc;
    if (B < 1) return gpmpc_refuse(who, "B < 1");
    if (H < 1) return gpmpc_refuse(who, "H < 1");
    if (!lpf_count_ok(B, H)) return gpmpc_refuse(who, "B x H is too large");
    if (flags & GPMPC_USE_GRAPH) return gpmpc_refuse(who, "GPMPC_USE_GRAPH is not supported by the linearised rollout (not yet)");
    if (flags & (GPMPC_FP32_ACCUM | GPMPC_FP32_ALL)) return gpmpc_refuse(who, "the GPMPC_FP32_* modes are not supported by the linearised rollout");
    if (flags & ~GPMPC_WANT_GRAD) return gpmpc_refuse(who, "flags: GPMPC_WANT_GRAD or 0");
    if (int rc = gpmpc_check_chunk(who, chunk)) return rc;
    const bool grad = (flags & GPMPC_WANT_GRAD) != 0;
    const int ds = m->state_dim, da = m->action_dim, p = lpf_p(ds);
    if (!x0 || !workspace || (da > 0 && !U)) return gpmpc_refuse(who, "NULL pointer");
    if (int rc = lpf_check_gain(who, m, K_dev, k_step_stride)) return rc;
    if (!lpf_sweep_fits(H, da)) return gpmpc_refuse(who, "H = %d is beyond the sweeps' grid (H da <= 64 x 65535)", H);
    if (out_jac && !grad) return gpmpc_refuse(who, "out_jac needs GPMPC_WANT_GRAD: without it no Jacobian is computed");
    if (cost && (!out_cost || (grad && !out_grad))) return gpmpc_refuse(who, "NULL pointer (out_cost, or out_grad with GPMPC_WANT_GRAD)");
    if (cons && (!out_g || (grad && !out_gjac))) return gpmpc_refuse(who, "NULL pointer (out_g, or out_gjac with GPMPC_WANT_GRAD)");
    if (cons) if (int rc = gpmpc_check_constraints(cons, who)) return rc;
    if (cons && da < 1) return gpmpc_refuse(who, "constraints need action_dim >= 1");
    if (cost) {
        if (da < 1) return gpmpc_refuse(who, "a cost needs action_dim >= 1");
        gpmpc_sched_ref sched;
        if (int rc = gpmpc_schedule_resolve(cost, ds, da, H, who, &sched)) return rc;
    }
    if (in) {
        if (in->input_cost && !cost) return gpmpc_refuse(who, "input_cost needs a cost: R is the cost's");
        if ((in->input_cost || in->ucons) && da < 1) return gpmpc_refuse(who, "the input cost and input constraints need action_dim >= 1");
        if (in->ucons) {
            if (int rc = gpmpc_lpi_check_rows(who, in->ucons)) return rc;
            if (!in->out_gu || (grad && !in->out_gujac)) return gpmpc_refuse(who, "NULL pointer (out_gu, or out_gujac with GPMPC_WANT_GRAD)");
            if (!grad && in->out_gujac) return gpmpc_refuse(who, "out_gujac needs GPMPC_WANT_GRAD: without it no Jacobian is computed");
        } else if (in->out_gu || in->out_gujac)
            return gpmpc_refuse(who, "out_gu / out_gujac without input constraints");
    }
    const LpfRollLayout R = lpf_roll_layout(m, B, H, grad, chunk);
    if (workspace_bytes < R.total) return GPMPC_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    double* means = out_means ? out_means : (double*)(ws + R.off_means);
    double* covs = out_covs ? out_covs : (double*)(ws + R.off_covs);
    double* jac = grad ? (out_jac ? out_jac : (double*)(ws + R.off_jac)) : nullptr;
    const size_t xs = (size_t)(H + 1) * ds, cs = xs * ds, jblock = (size_t)p * (p + da), js = (size_t)H * jblock;
    GPMPC_HIP(hipMemsetAsync(ws + R.step.off_zero, 0, R.step.zero_bytes, s));
    hipLaunchKernelGGL(k_lpf_init, dim3(gpmpc_blocks256((long)B * (ds + ds * ds))), dim3(256), 0, s, B, H, ds, x0, M.noise, means, covs);
    for (int t = 1; t <= H; ++t) {
        const double* K_t = K_dev ? K_dev + (size_t)(t - 1) * k_step_stride : nullptr;
        if (int rc = lpf_step(m, M, B, means + (size_t)(t - 1) * ds, xs, covs + (size_t)(t - 1) * ds * ds, cs, U ? U + (size_t)(t - 1) * da : nullptr,
                              (size_t)H * da, K_t, means + (size_t)t * ds, xs, covs + (size_t)t * ds * ds, cs,
                              jac ? jac + (size_t)(t - 1) * jblock : nullptr, js, R.step, ws, s))
            return rc;
    }
    if (cost) {
        double *dm = grad ? (double*)(ws + R.off_dm) : nullptr, *dc = grad ? (double*)(ws + R.off_dc) : nullptr;
        double* du = grad ? (double*)(ws + R.off_du) : nullptr;
        if (int rc = gpmpc_cost_grad(B, H, ds, da, cost, means, covs, U, out_cost, dm, dc, du, stream)) return rc;
        if (in && in->input_cost)
            if (int rc = gpmpc_lpi_cost(B, H, ds, da, cost, K_dev, k_step_stride, covs, nullptr, nullptr, out_cost, dc, s)) return rc;
        if (grad)
            hipLaunchKernelGGL(k_lpf_vjp, dim3(B), dim3(64), 0, s, H, ds, da, (const double*)jac, (const double*)dm, (const double*)dc,
                               (const double*)du, out_grad, (double*)nullptr);
    }
    if (cons)
        if (int rc = lpf_constraints(B, H, ds, da, cons, means, covs, grad ? jac : nullptr, out_g, grad ? out_gjac : nullptr, s)) return rc;
    if (in && in->ucons)
        if (int rc = gpmpc_lpi_constraints(B, H, ds, da, in->ucons, K_dev, k_step_stride, U, covs, grad ? jac : nullptr, in->out_gu,
                                           grad ? in->out_gujac : nullptr, s))
            return rc;
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}
