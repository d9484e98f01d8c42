// The risk-sensitive cost for given means / FULL covariances (gpmpc_cost, gpmpc_cost_grad) and the vector-Jacobian product of the
// rollout (gpmpc_rollout_vjp): stand-alone kernels, none of the rollout's types.  The tail kernel's register-resident cost terms for
// a diagonal covariance are in step.hip.
#include "gpmpc_internal.h"

// ---------------------------------------------------------------------------
// cost (src/mpc.py:179-198) and its derivatives
// ---------------------------------------------------------------------------
// Per-step state cost with a general (possibly non-symmetric) covariance Sig [ds][ds]:
//   (1/gamma) log det(I + gamma Q Sig) + e^T (Q^-1 + gamma Sig)^-1 e,   e = mu - x_ref.
// (Q^-1 + gamma Sig)^-1 = (I + gamma Q Sig)^-1 Q =: Z, so one LU of Mx = I + gamma Q Sig gives the
// determinant and Z (no inverse of Q is formed).  Optionally returns d/dmu and d/dSig_kk.
// w: scratch, ds * 2ds doubles.  gamma == 0: tr(Q Sig) + e^T Q e.
// dsig (optional, [ds][ds], general Sigma): d/dSig_kl = Z_lk - gamma (Z^T e)_k (Z e)_l -- what autograd returns for the
// reference's expression with a non-symmetric Sig (src/mpc.py:182-185).
__device__ static double state_cost(int ds, const gpmpc_cost_params& C, const double* mu, const double* Sig, int sig_ld,
                                    bool sig_diag, double* w, double* dmu, double* dvar, double* dsig = nullptr) {
    const double g = C.gamma;
    double e[GPMPC_MAX_DS];
    for (int k = 0; k < ds; ++k) e[k] = mu[k] - C.x_ref[k];
    if (g == 0.0) {
        double c = 0.0;
        for (int k = 0; k < ds; ++k) {
            double qe = 0.0;
            for (int l = 0; l < ds; ++l) {
                qe += C.Q[k * ds + l] * e[l];
                const double sig_lk = sig_diag ? (l == k ? Sig[k] : 0.0) : Sig[l * sig_ld + k];
                c += C.Q[k * ds + l] * sig_lk;
            }
            c += e[k] * qe;
            if (dmu) {
                double qte = 0.0;
                for (int l = 0; l < ds; ++l) qte += C.Q[l * ds + k] * e[l];
                dmu[k] = qe + qte;
                if (dvar) dvar[k] = C.Q[k * ds + k];
                if (dsig) for (int l = 0; l < ds; ++l) dsig[k * ds + l] = C.Q[l * ds + k];
            }
        }
        return c;
    }
    const int ld = 2 * ds;     // augmented [Mx | Q]
    for (int r = 0; r < ds; ++r)
        for (int cc = 0; cc < ds; ++cc) {
            double s = 0.0;
            if (sig_diag) s = C.Q[r * ds + cc] * Sig[cc];
            else for (int l = 0; l < ds; ++l) s += C.Q[r * ds + l] * Sig[l * sig_ld + cc];
            w[r * ld + cc] = (r == cc ? 1.0 : 0.0) + g * s;
            w[r * ld + ds + cc] = C.Q[r * ds + cc];
        }
    double det = 1.0;
    for (int k = 0; k < ds; ++k) {           // Gauss-Jordan with partial pivoting
        int piv = k; double best = fabs(w[k * ld + k]);
        for (int r = k + 1; r < ds; ++r) { const double v = fabs(w[r * ld + k]); if (v > best) { best = v; piv = r; } }
        if (piv != k) {
            for (int cc = 0; cc < ld; ++cc) { const double tmp = w[k * ld + cc]; w[k * ld + cc] = w[piv * ld + cc]; w[piv * ld + cc] = tmp; }
            det = -det;
        }
        const double pv = w[k * ld + k];
        det *= pv;
        const double inv = 1.0 / pv;
        for (int cc = 0; cc < ld; ++cc) w[k * ld + cc] *= inv;
        for (int r = 0; r < ds; ++r) {
            if (r == k) continue;
            const double f = w[r * ld + k];
            for (int cc = 0; cc < ld; ++cc) w[r * ld + cc] = fma(-f, w[k * ld + cc], w[r * ld + cc]);
        }
    }
    // Z = w[:, ds:]
    double ze[GPMPC_MAX_DS], zte[GPMPC_MAX_DS], quad = 0.0;
    for (int k = 0; k < ds; ++k) {
        double s = 0.0, st = 0.0;
        for (int l = 0; l < ds; ++l) { s += w[k * ld + ds + l] * e[l]; st += w[l * ld + ds + k] * e[l]; }
        ze[k] = s; zte[k] = st;
        quad += e[k] * s;
    }
    if (dmu)
        for (int k = 0; k < ds; ++k) {
            dmu[k] = ze[k] + zte[k];
            if (dvar) dvar[k] = w[k * ld + ds + k] - g * zte[k] * ze[k];
            if (dsig) for (int l = 0; l < ds; ++l) dsig[k * ds + l] = w[l * ld + ds + k] - g * zte[k] * ze[l];
        }
    return log(det) / g + quad;
}

// Input-cost terms (src/mpc.py:188-198) for one trajectory; optionally accumulates d/dU into gU [H][da].
// uref_rows: SCHED: the [H][da] input references of a cost schedule; else not read (C.u_ref at every step)
template <bool SCHED>
__device__ static double input_cost(int H, int da, const gpmpc_cost_params& C, const double* uref_rows, const double* U, double* gU) {
    double c = 0.0;
    for (int j = 0; j < H; ++j) {
        double d[GPMPC_MAX_D];
        const double* ur = SCHED ? uref_rows + (size_t)j * da : C.u_ref;
        for (int k = 0; k < da; ++k) d[k] = U[j * da + k] - ur[k];
        for (int k = 0; k < da; ++k) {
            double rd = 0.0, rtd = 0.0;
            for (int l = 0; l < da; ++l) { rd += C.R[k * da + l] * d[l]; rtd += C.R[l * da + k] * d[l]; }
            c += d[k] * rd;
            if (gU) gU[j * da + k] += rd + rtd;
        }
        if (C.has_R_delta) {
            for (int k = 0; k < da; ++k) d[k] = U[j * da + k] - (j == 0 ? C.last_u[k] : U[(j - 1) * da + k]);
            for (int k = 0; k < da; ++k) {
                double rd = 0.0, rtd = 0.0;
                for (int l = 0; l < da; ++l) { rd += C.R_delta[k * da + l] * d[l]; rtd += C.R_delta[l * da + k] * d[l]; }
                c += d[k] * rd;
                if (gU) { gU[j * da + k] += rd + rtd; if (j > 0) gU[(j - 1) * da + k] -= rd + rtd; }
            }
        }
    }
    return c;
}

// Stand-alone cost for given means / FULL covariances (cost_torch parity, src/mpc.py:156-200).
// d_means / d_covs / d_U (all or none): the analytic derivatives autograd takes of the reference's expression
// (src/mpc.py:251 backward through :179-198), for the differentiable cost_torch of the host mirror.
__global__ void k_cost_full(int B, int H, int ds, int da, gpmpc_cost_params C, const double* means, const double* covs,
                            const double* U, double* out, double* d_means, double* d_covs, double* d_U) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double w[GPMPC_MAX_DS * 2 * GPMPC_MAX_DS];
    double total = 0.0;
    for (int i = 0; i <= H; ++i) {
        const size_t o = (size_t)b * (H + 1) + i;
        total += state_cost(ds, C, means + o * ds, covs + o * ds * ds, ds, false, w, d_means ? d_means + o * ds : nullptr,
                            nullptr, d_means ? d_covs + o * ds * ds : nullptr);
    }
    if (d_U) for (int q = 0; q < H * da; ++q) d_U[(size_t)b * H * da + q] = 0.0;
    total += input_cost<false>(H, da, C, nullptr, U + (size_t)b * H * da, d_U ? d_U + (size_t)b * H * da : nullptr);
    out[b] = total;
}

// state_cost with the state dimension known at compile time and the reference and weight of THIS step as arguments (xref [DS],
// Qw [DS][DS]): the same operations in the same order, the elimination in registers (row swaps as predicated moves).  For the schedule
// variant of the stand-alone cost below.
template <int DS>
__device__ static double state_cost_sched(const double g, const double* __restrict__ xref, const double* __restrict__ Qw,
                                          const double* __restrict__ mu, const double* __restrict__ Sig, double* dmu, double* dsig) {
    double e[DS], sg[DS][DS], Q[DS][DS];
#pragma unroll
    for (int k = 0; k < DS; ++k) {
        e[k] = mu[k] - xref[k];
#pragma unroll
        for (int l = 0; l < DS; ++l) { sg[k][l] = Sig[k * DS + l]; Q[k][l] = Qw[k * DS + l]; }
    }
    if (g == 0.0) {
        double c = 0.0;
#pragma unroll
        for (int k = 0; k < DS; ++k) {
            double qe = 0.0, qte = 0.0;
#pragma unroll
            for (int l = 0; l < DS; ++l) { qe += Q[k][l] * e[l]; c += Q[k][l] * sg[l][k]; }
            c += e[k] * qe;
            if (dmu) {
#pragma unroll
                for (int l = 0; l < DS; ++l) qte += Q[l][k] * e[l];
                dmu[k] = qe + qte;
#pragma unroll
                for (int l = 0; l < DS; ++l) dsig[k * DS + l] = Q[l][k];
            }
        }
        return c;
    }
    double w[DS][2 * DS];          // augmented [I + gamma Q Sig | Q]
#pragma unroll
    for (int r = 0; r < DS; ++r)
#pragma unroll
        for (int cc = 0; cc < DS; ++cc) {
            double s = 0.0;
#pragma unroll
            for (int l = 0; l < DS; ++l) s += Q[r][l] * sg[l][cc];
            w[r][cc] = (r == cc ? 1.0 : 0.0) + g * s;
            w[r][DS + cc] = Q[r][cc];
        }
    double det = 1.0;
#pragma unroll
    for (int k = 0; k < DS; ++k) {           // Gauss-Jordan with partial pivoting
        int piv = k;
        double best = fabs(w[k][k]);
#pragma unroll
        for (int r = k + 1; r < DS; ++r) { const double v = fabs(w[r][k]); if (v > best) { best = v; piv = r; } }
#pragma unroll
        for (int r = k + 1; r < DS; ++r) {
            const bool sw = piv == r;
#pragma unroll
            for (int cc = 0; cc < 2 * DS; ++cc) {
                const double a = w[k][cc], bb = w[r][cc];
                w[k][cc] = sw ? bb : a;
                w[r][cc] = sw ? a : bb;
            }
        }
        if (piv != k) det = -det;
        const double pv = w[k][k];
        det *= pv;
        const double inv = 1.0 / pv;
#pragma unroll
        for (int cc = 0; cc < 2 * DS; ++cc) w[k][cc] *= inv;
#pragma unroll
        for (int r = 0; r < DS; ++r) {
            if (r == k) continue;
            const double f = w[r][k];
#pragma unroll
            for (int cc = 0; cc < 2 * DS; ++cc) w[r][cc] = fma(-f, w[k][cc], w[r][cc]);
        }
    }
    double ze[DS], zte[DS], quad = 0.0;
#pragma unroll
    for (int k = 0; k < DS; ++k) {
        double s = 0.0, st = 0.0;
#pragma unroll
        for (int l = 0; l < DS; ++l) { s += w[k][DS + l] * e[l]; st += w[l][DS + k] * e[l]; }
        ze[k] = s; zte[k] = st;
        quad += e[k] * s;
    }
    if (dmu) {
#pragma unroll
        for (int k = 0; k < DS; ++k) {
            dmu[k] = ze[k] + zte[k];
#pragma unroll
            for (int l = 0; l < DS; ++l) dsig[k * DS + l] = w[l][DS + k] - g * zte[k] * ze[l];
        }
    }
    return log(det) / g + quad;
}

// k_cost_full with a cost schedule (include/gpmpc.h): step i measures mu_i against row i of the schedule, step H under Q_f where one is
// set, input j against u_ref[j].  One thread per trajectory, like k_cost_full; the derivative outputs are written straight to memory.
template <int DS>
__global__ __launch_bounds__(64) void k_cost_sched(int B, int H, int da, gpmpc_cost_params C, const double* __restrict__ sched, int H_max,
                                                   const double* __restrict__ means, const double* __restrict__ covs,
                                                   const double* __restrict__ U, double* out, double* d_means, double* d_covs, double* d_U) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double total = 0.0;
    for (int i = 0; i <= H; ++i) {
        const size_t o = (size_t)b * (H + 1) + i;
        double xr[DS], Qw[DS * DS];
        const double* __restrict__ xs = sched + (size_t)i * DS;
#pragma unroll
        for (int k = 0; k < DS; ++k) xr[k] = xs[k];
#pragma unroll
        for (int q = 0; q < DS * DS; ++q) Qw[q] = C.Q[q];
        if (i == H) {
            const double* __restrict__ qf = sched + gpmpc_sched_off_q(H_max, DS, da);
            const double has = qf[DS * DS];
#pragma unroll
            for (int q = 0; q < DS * DS; ++q) { const double v = qf[q]; Qw[q] = has != 0.0 ? v : Qw[q]; }
        }
        total += state_cost_sched<DS>(C.gamma, xr, Qw, means + o * DS, covs + o * DS * DS, d_means ? d_means + o * DS : nullptr,
                                      d_means ? d_covs + o * DS * DS : nullptr);
    }
    if (d_U) for (int q = 0; q < H * da; ++q) d_U[(size_t)b * H * da + q] = 0.0;
    total += input_cost<true>(H, da, C, sched + gpmpc_sched_off_u(H_max, DS), U + (size_t)b * H * da, d_U ? d_U + (size_t)b * H * da : nullptr);
    out[b] = total;
}

// Vector-Jacobian product of the rollout (the backward pass of forward_propagate_torch's autograd graph,
// src/dynamics.py:126-191 under src/mpc.py:251): reverse sweep over the step Jacobians J_t [2ds][2ds+da] (rows: mu_t, var_t;
// columns: mu_{t-1}, var_{t-1}, u_{t-1}) seeded with the upstream gradients of EVERY step's mean and variance.
// One wave per trajectory; lane c owns column c.
__global__ __launch_bounds__(64) void k_rollout_vjp(int B, int H, int ds, int da, const double* __restrict__ jac,
                                                    const double* __restrict__ g_means, const double* __restrict__ g_vars,
                                                    double* __restrict__ out_gU, double* __restrict__ out_gx0) {
    __shared__ double s_adj[2][2 * GPMPC_MAX_DS];
    const int b = blockIdx.x, c = threadIdx.x, nz = 2 * ds, nc = 2 * ds + da;
    auto seed = [&](int t, int r) {
        const size_t o = ((size_t)b * (H + 1) + t) * ds;
        return r < ds ? (g_means ? g_means[o + r] : 0.0) : (g_vars ? g_vars[o + (r - ds)] : 0.0);
    };
    if (c < nz) s_adj[0][c] = seed(H, c);
    __syncthreads();
    int cur = 0;
    for (int t = H; t >= 1; --t) {
        const double* Jt = jac + ((size_t)b * H + (t - 1)) * nz * nc;
        if (c < nc) {
            double sum = 0.0;
            for (int r = 0; r < nz; ++r) sum = fma(Jt[r * nc + c], s_adj[cur][r], sum);
            if (c < nz) s_adj[cur ^ 1][c] = seed(t - 1, c) + sum;
            else out_gU[((size_t)b * H + (t - 1)) * da + (c - nz)] = sum;
        }
        __syncthreads();
        cur ^= 1;
    }
    if (out_gx0 && c < ds) out_gx0[(size_t)b * ds + c] = s_adj[cur][c];      // mu_0 = x0; Sigma_0 is a constant
}

extern "C" int gpmpc_cost_grad(int B, int H, int ds, int da, const gpmpc_cost_params* cost, const double* means,
                               const double* covs, const double* U, double* out_cost, double* d_means, double* d_covs,
                               double* d_U, void* stream) {
    if (!cost || !means || !covs || !U || !out_cost || B < 1 || H < 1 || ds < 1 || ds > GPMPC_MAX_DS || da < 0 ||
        da > GPMPC_MAX_D)
        return GPMPC_E_ARG;
    const int ng = (d_means != nullptr) + (d_covs != nullptr) + (d_U != nullptr);
    if (ng != 0 && ng != 3) return GPMPC_E_ARG;            // all three derivative outputs or none
    gpmpc_sched_ref sched;
    if (int rcs = gpmpc_schedule_resolve(cost, ds, da, H, "gpmpc_cost", &sched)) return rcs;
    if (sched.dev) {
        if (int rc = gpmpc_dispatch_dim<1>(ds, [&](auto d) {
                hipLaunchKernelGGL(k_cost_sched<decltype(d)::value>, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, H, da, *cost,
                                   sched.dev, sched.H_max, means, covs, U, out_cost, d_means, d_covs, d_U);
                return GPMPC_OK;
            }))
            return rc;
        GPMPC_HIP(hipGetLastError());
        return GPMPC_OK;
    }
    hipLaunchKernelGGL(k_cost_full, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, H, ds, da, *cost, means,
                       covs, U, out_cost, d_means, d_covs, d_U);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

extern "C" int gpmpc_cost(int B, int H, int ds, int da, const gpmpc_cost_params* cost, const double* means,
                          const double* covs, const double* U, double* out_cost, void* stream) {
    return gpmpc_cost_grad(B, H, ds, da, cost, means, covs, U, out_cost, nullptr, nullptr, nullptr, stream);
}

extern "C" int gpmpc_rollout_vjp(int B, int H, int ds, int da, const double* jac, const double* g_means,
                                 const double* g_vars, double* out_gU, double* out_gx0, void* stream) {
    if (!jac || !out_gU || B < 1 || H < 1 || ds < 1 || ds > GPMPC_MAX_DS || da < 1 || da > GPMPC_MAX_D || 2 * ds + da > 64)
        return GPMPC_E_ARG;
    hipLaunchKernelGGL(k_rollout_vjp, dim3(B), dim3(64), 0, (hipStream_t)stream, B, H, ds, da, jac, g_means, g_vars, out_gU,
                       out_gx0);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}
