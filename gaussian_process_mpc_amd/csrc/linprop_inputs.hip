// The commanded input under a linear state feedback, u_t = v_t + K_t (x_t - mu_t) ~ N(v_t, K_t Sigma_t K_t^T): its cost and its chance
// constraints on the full-covariance linearised rollout.  Formulas, layouts and refusals: include/gpmpc.h, "Linearised propagation, full
// covariance: the commanded input"; the why: DESIGN.md section 3n.
//   k_lpi_cost          one workgroup per plan: c = sum_j tr(R K_j Sigma_j K_j^T) and its derivative by Sigma_j, steps in ascending order
//   k_lpi_constraints   the forward-sensitivity sweep of k_lpf_constraints (linprop_fc.hip), evaluated on the state BEFORE each step:
//                       g_u[t][r] = c_r . v_t + kappa_r sqrt(a^T Sigma_t a) - d_r, a = K_t^T c_r, and its dense Jacobian
//   k_lpi_pinputs       particles under the same feedback: u^p = v_b + K_t (x^p - mu_b), one thread per (particle, input)
//   k_lpi_assemble      k_pt_assemble (particles.hip) with an input per particle
//   k_lpi_ustats, k_lpi_ujoint   mean, covariance and violation fractions of the particles' inputs, by the rules of k_pt_stats / k_pt_joint
// Rules: no atomics; launch geometry from the sizes only; every output element is written; two identical calls agree bit for bit.
#include <cmath>
#include "linprop_internal.h"
#include "philox.h"                 // MPPI_THREADS and the fixed-order folds of the particle statistics
#include "particles_internal.h"

#define LPI_MAX_TRI (GPMPC_MAX_DS * (GPMPC_MAX_DS + 1) / 2)
#define LPI_MAX_P (GPMPC_MAX_DS + LPI_MAX_TRI)

struct LpiR { double R[GPMPC_MAX_D * GPMPC_MAX_D]; };

// grid (B), 64 threads.  covs [B][H+1][ds][ds], every entry read as given (the convention of gpmpc_cost_grad: a general matrix).
// Mm[k][l] = sum_{a,b} K_al R_ab K_bk = d c / d Sigma_j[k][l].  out_c / out_dcovs / add_cost / add_dcovs: any may be null.
__global__ __launch_bounds__(64) void k_lpi_cost(int H, int ds, int da, LpiR Rm, const double* __restrict__ K, size_t kss,
                                                 const double* __restrict__ covs, double* __restrict__ out_c, double* __restrict__ out_dcovs,
                                                 double* __restrict__ add_cost, double* __restrict__ add_dcovs) {
    constexpr int M = GPMPC_MAX_D;
    __shared__ double Kg[M][M], RK[M][M], term[M * M];
    const int b = blockIdx.x, t = threadIdx.x, n2 = ds * ds;
    const int k = t / ds, l = t - k * ds;                   // of the threads t < ds ds
    double acc = 0.0, m = 0.0;
    for (int j = 0; j < H; ++j) {
        if (K && (j == 0 || kss != 0)) {
            __syncthreads();
            for (int e = t; e < da * ds; e += 64) Kg[e / ds][e % ds] = K[(size_t)j * kss + e];
            __syncthreads();
            for (int e = t; e < da * ds; e += 64) {
                const int a = e / ds, kk = e - a * ds;
                double s = 0.0;
                for (int bb = 0; bb < da; ++bb) s = fma(Rm.R[a * da + bb], Kg[bb][kk], s);
                RK[a][kk] = s;
            }
            __syncthreads();
            if (t < n2) {
                double s = 0.0;
                for (int a = 0; a < da; ++a) s = fma(Kg[a][l], RK[a][k], s);
                m = s;
            }
        }
        const size_t o = ((size_t)b * (H + 1) + j) * n2 + t;
        if (t < n2) {
            term[t] = K ? m * covs[o] : 0.0;
            if (out_dcovs) out_dcovs[o] = m;
            if (add_dcovs) add_dcovs[o] = add_dcovs[o] + m;
        }
        __syncthreads();
        if (t == 0) {
            double s = 0.0;
            for (int e = 0; e < n2; ++e) s += term[e];
            acc += s;
        }
        __syncthreads();
    }
    if (t < n2) {                                                                     // Sigma_H meets no input
        const size_t o = ((size_t)b * (H + 1) + H) * n2 + t;
        if (out_dcovs) out_dcovs[o] = 0.0;
        if (add_dcovs) add_dcovs[o] = add_dcovs[o] + 0.0;
    }
    if (t == 0) {
        if (out_c) out_c[b] = acc;
        if (add_cost) add_cost[b] = add_cost[b] + acc;
    }
}

// grid (B, ceil(H da / 64)), one wave per workgroup, lane = column tau da + j of the dense Jacobian; the column's p sensitivities live in
// LDS, [row][lane]: the geometry and the propagation of k_lpf_constraints.  Row t is evaluated on S_t, the sensitivities of the packed state
// of step t before the step is taken (S_0 = 0).  JAC = false: values only (grid (B, 1)).
template <int DS, bool JAC>
__global__ __launch_bounds__(64) void k_lpi_constraints(int H, int da, gpmpc_input_constraints C, const double* __restrict__ K, size_t kss,
                                                        const double* __restrict__ U, const double* __restrict__ covs,
                                                        const double* __restrict__ jac, double* __restrict__ out_gu,
                                                        double* __restrict__ out_gujac) {
    constexpr int NT = DS * (DS + 1) / 2, NP = DS + NT;
    __shared__ double S[JAC ? 2 : 1][JAC ? NP : 1][64];
    const int b = blockIdx.x, lane = threadIdx.x, mu = C.n_rows, nc = NP + da, ncols = H * da;
    const int c0 = blockIdx.y * 64, c = c0 + lane;
    const bool live = c < ncols;
    const int tau = c / da, j = c - tau * da, tau0 = c0 / da;
    const bool first = blockIdx.y == 0;
    int cur = 0;
    if (JAC)
        for (int r = 0; r < NP; ++r) S[0][JAC ? r : 0][lane] = 0.0;
    for (int t = 0; t < H; ++t) {
        if (JAC && t >= 1 && tau0 < t) {
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
        const double* __restrict__ v = U + ((size_t)b * H + t) * da;
        const double* __restrict__ cv = covs + ((size_t)b * (H + 1) + t) * DS * DS;
        const double* __restrict__ Kt = K ? K + (size_t)t * kss : nullptr;
        for (int r = 0; r < mu; ++r) {
            double a[DS];
#pragma unroll
            for (int k = 0; k < DS; ++k) a[k] = 0.0;
            double cm = 0.0;
            for (int i = 0; i < da; ++i) {
                const double ci = C.C[r * da + i];
                cm = fma(ci, v[i], cm);
                if (Kt) {
#pragma unroll
                    for (int k = 0; k < DS; ++k) a[k] = fma(ci, Kt[i * DS + k], a[k]);
                }
            }
            double q = 0.0;
            if (Kt) {
#pragma unroll
                for (int k = 0; k < DS; ++k)
#pragma unroll
                    for (int l = 0; l < DS; ++l) q = fma(a[k] * a[l], cv[k * DS + l], q);
            }
            // q <= 0: sd = 0 and no variance part; NaN passes through
            const double sd = q > 0.0 ? sqrt(q) : (q <= 0.0 ? 0.0 : q);
            const double kap = C.kappa[r];
            if (first && lane == 0) out_gu[((size_t)b * H + t) * mu + r] = fma(kap, sd, cm) - C.d[r];
            if (JAC) {
                const double f = q <= 0.0 ? 0.0 : kap / (2.0 * sd);
                double dv = 0.0;
                int vv = DS;
#pragma unroll
                for (int k = 0; k < DS; ++k) {
#pragma unroll
                    for (int l = k; l < DS; ++l, ++vv) {    // the variable Sigma_kl stands for both entries (k, l) and (l, k)
                        const double w = k == l ? a[k] * a[k] : 2.0 * (a[k] * a[l]);
                        dv = fma(w, S[JAC ? cur : 0][JAC ? vv : 0][lane], dv);
                    }
                }
                if (live) out_gujac[(((size_t)b * H + t) * mu + r) * ncols + c] = tau < t ? f * dv : (tau == t ? C.C[r * da + j] : 0.0);
            }
        }
    }
}

struct LpiSd { double v[GPMPC_MAX_D]; };

// one thread per (c = b P + p, j): out_u[c][j] = v_b[j] + sum_k K[j][k] (x[c][k] - mu_b[k]), k ascending; K null: a copy of v_b[j]
__global__ __launch_bounds__(256) void k_lpi_pinputs(int B, int P, int ds, int da, const double* __restrict__ x, const double* __restrict__ U,
                                                     size_t us, const double* __restrict__ K, const double* __restrict__ mu, size_t ms,
                                                     double* __restrict__ out_u) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B * P * da) return;
    const int j = (int)(e % da);
    const long c = e / da;
    const int b = (int)(c / P);
    const double v = U[(size_t)b * us + j];
    if (!K) { out_u[e] = v; return; }
    double s = 0.0;
    for (int k = 0; k < ds; ++k) s = fma(K[j * ds + k], x[(size_t)c * ds + k] - mu[(size_t)b * ms + k], s);
    out_u[e] = v + s;
}

// z[c] = (x_prev[c], U_p[c] + sqrt(action_var) eps_u[p]): k_pt_assemble with the input of particle c in the place of the plan's
__global__ __launch_bounds__(256) void k_lpi_assemble(int B, int P, int ds, int da, const double* __restrict__ x_prev,
                                                      const double* __restrict__ U_p, const double* __restrict__ eps, LpiSd sd,
                                                      double* __restrict__ z) {
    const int D = ds + da;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B * P * D) return;
    const int d = (int)(e % D);
    const long c = e / D;
    const int p = (int)(c % P);
    z[e] = d < ds ? x_prev[(size_t)c * ds + d] : U_p[(size_t)c * da + (d - ds)] + sd.v[d - ds] * eps[(size_t)p * D + (d - ds)];
}

// grid (H, B).  Thread i adds the particles i, i + 256, ... in ascending order; the 256 partial sums are folded in halves (k_pt_stats).
__global__ __launch_bounds__(MPPI_THREADS) void k_lpi_ustats(int B, int P, int H, int da, const double* __restrict__ X, int n_rows,
                                                             gpmpc_input_constraints cons, double* __restrict__ out_mean,
                                                             double* __restrict__ out_cov, double* __restrict__ out_viol) {
    __shared__ double red[MPPI_THREADS];
    __shared__ int redi[MPPI_THREADS];
    const int tid = threadIdx.x, t = blockIdx.x, b = blockIdx.y;
    const double* __restrict__ x = X + ((size_t)t * B + b) * P * da;
    double mean[GPMPC_MAX_D];
#pragma unroll
    for (int e = 0; e < GPMPC_MAX_D; ++e) {
        mean[e] = 0.0;
        if (e < da) {
            double s = 0.0;
            for (int p = tid; p < P; p += MPPI_THREADS) s = s + x[(size_t)p * da + e];
            mean[e] = mppi_fold_sum(s, red) / (double)P;
            if (out_mean && tid == 0) out_mean[((size_t)b * H + t) * da + e] = mean[e];
        }
    }
    if (out_cov) {
#pragma unroll
        for (int e = 0; e < GPMPC_MAX_D; ++e)
#pragma unroll
            for (int f = e; f < GPMPC_MAX_D; ++f) {
                if (f >= da) continue;
                double s = 0.0;
                for (int p = tid; p < P; p += MPPI_THREADS) s = s + (x[(size_t)p * da + e] - mean[e]) * (x[(size_t)p * da + f] - mean[f]);
                const double cv = mppi_fold_sum(s, red) / (double)(P - 1);
                if (tid == 0) {
                    double* o = out_cov + ((size_t)b * H + t) * da * da;
                    o[e * da + f] = cv;
                    o[f * da + e] = cv;
                }
            }
    }
    for (int r = 0; r < n_rows; ++r) {
        int cnt = 0;
        for (int p = tid; p < P; p += MPPI_THREADS) {
            double g = 0.0;
            for (int e = 0; e < da; ++e) g = g + cons.C[r * da + e] * x[(size_t)p * da + e];
            cnt += g > cons.d[r] ? 1 : 0;
        }
        cnt = mppi_fold_count(cnt, redi);
        if (tid == 0) out_viol[((size_t)b * H + t) * n_rows + r] = (double)cnt / (double)P;
    }
}

// grid (B): the fraction of particles whose input violates some row at some step t = 0 ... H-1
__global__ __launch_bounds__(MPPI_THREADS) void k_lpi_ujoint(int B, int P, int H, int da, const double* __restrict__ X, int n_rows,
                                                             gpmpc_input_constraints cons, double* __restrict__ out_joint) {
    __shared__ int redi[MPPI_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    int cnt = 0;
    for (int p = tid; p < P; p += MPPI_THREADS) {
        bool any = false;
        for (int t = 0; t < H; ++t) {
            const double* __restrict__ x = X + (((size_t)t * B + b) * P + p) * da;
            for (int r = 0; r < n_rows; ++r) {
                double g = 0.0;
                for (int e = 0; e < da; ++e) g = g + cons.C[r * da + e] * x[e];
                any |= g > cons.d[r];
            }
        }
        cnt += any ? 1 : 0;
    }
    cnt = mppi_fold_count(cnt, redi);
    if (tid == 0) out_joint[b] = (double)cnt / (double)P;
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
static bool lpi_count_ok(long B, long H) { return B >= 1 && H >= 1 && B * H * (long)LPI_MAX_P * (LPI_MAX_P + GPMPC_MAX_D) <= (1L << 40); }
static bool lpi_sweep_fits(long H, int da) { return H * (da > 0 ? da : 1) <= 64L * 65535; }

// the checks of gpmpc_check_constraints on the input rows
int gpmpc_lpi_check_rows(const char* who, const gpmpc_input_constraints* C) {
    if (!C) return gpmpc_refuse(who, "NULL pointer (input constraints)");
    if (C->n_rows < 1 || C->n_rows > GPMPC_MAX_CONS) return gpmpc_refuse(who, "input constraints: n_rows = %d outside 1..%d", C->n_rows, GPMPC_MAX_CONS);
    for (int r = 0; r < C->n_rows; ++r)
        if (!(C->kappa[r] >= 0.0)) return gpmpc_refuse(who, "input constraints: kappa[%d] = %g is negative or NaN", r, C->kappa[r]);
    return GPMPC_OK;
}

int gpmpc_lpi_cost(int B, int H, int ds, int da, const gpmpc_cost_params* cost, const double* K, size_t k_step_stride, const double* covs,
                   double* out_c, double* out_dcovs, double* add_cost, double* add_dcovs, hipStream_t s) {
    LpiR Rm;
    memset(&Rm, 0, sizeof(Rm));
    memcpy(Rm.R, cost->R, sizeof(double) * da * da);
    hipLaunchKernelGGL(k_lpi_cost, dim3(B), dim3(64), 0, s, H, ds, da, Rm, K, k_step_stride, covs, out_c, out_dcovs, add_cost, add_dcovs);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

int gpmpc_lpi_constraints(int B, int H, int ds, int da, const gpmpc_input_constraints* C, const double* K, size_t k_step_stride,
                          const double* U, const double* covs, const double* jac, double* out_gu, double* out_gujac, hipStream_t s) {
    if (int rc = gpmpc_dispatch_dim<1>(ds, [&](auto d) {
            constexpr int DS = decltype(d)::value;
            if (out_gujac)
                hipLaunchKernelGGL((k_lpi_constraints<DS, true>), dim3(B, (H * da + 63) / 64), dim3(64), 0, s, H, da, *C, K, k_step_stride, U, covs, jac,
                                   out_gu, out_gujac);
            else
                hipLaunchKernelGGL((k_lpi_constraints<DS, false>), dim3(B, 1), dim3(64), 0, s, H, da, *C, K, k_step_stride, U, covs, jac, out_gu,
                                   out_gujac);
            return GPMPC_OK;
        }))
        return rc;
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

// what the pure functions refuse of the sizes and of the gain
static int lpi_check_sizes(const char* who, int B, int H, int ds, int da, size_t k_step_stride) {
    if (B < 1 || H < 1) return gpmpc_refuse(who, "B or H < 1");
    if (ds < 1 || ds > GPMPC_MAX_DS || da < 1 || ds + da > GPMPC_MAX_D) return gpmpc_refuse(who, "state_dim or action_dim outside the range");
    if (!lpi_count_ok(B, H) || !lpi_sweep_fits(H, da)) return gpmpc_refuse(who, "H = %d is beyond the sweep's grid (H da <= 64 x 65535)", H);
    if (k_step_stride != 0 && k_step_stride != (size_t)da * ds) return gpmpc_refuse(who, "k_step_stride must be 0 or action_dim state_dim");
    return GPMPC_OK;
}

extern "C" int gpmpc_feedback_input_cost(int B, int H, int ds, int da, const gpmpc_cost_params* cost, const double* K_dev, size_t k_step_stride,
                                         const double* covs, double* out_c, double* out_dcovs, void* stream) {
    const char* who = "gpmpc_feedback_input_cost";
    if (!cost || !covs || !out_c) return gpmpc_refuse(who, "NULL pointer");
    if (int rc = lpi_check_sizes(who, B, H, ds, da, k_step_stride)) return rc;
    return gpmpc_lpi_cost(B, H, ds, da, cost, K_dev, k_step_stride, covs, out_c, out_dcovs, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int gpmpc_feedback_input_constraints(int B, int H, int ds, int da, const gpmpc_input_constraints* C, const double* K_dev,
                                                size_t k_step_stride, const double* U, const double* covs, const double* jac, double* out_gu,
                                                double* out_gujac, void* stream) {
    const char* who = "gpmpc_feedback_input_constraints";
    if (!C || !U || !covs || !out_gu || (out_gujac && !jac)) return gpmpc_refuse(who, "NULL pointer");
    if (int rc = lpi_check_sizes(who, B, H, ds, da, k_step_stride)) return rc;
    if (int rc = gpmpc_lpi_check_rows(who, C)) return rc;
    return gpmpc_lpi_constraints(B, H, ds, da, C, K_dev, k_step_stride, U, covs, jac, out_gu, out_gujac, (hipStream_t)stream);
}

// The workspace is that of gpmpc_linearised_fc_rollout: the input statistics keep nothing beside the caller's arrays.
extern "C" size_t gpmpc_linearised_fc_rollout_inputs_workspace_bytes(const gpmpc_gp_model* m, int B, int H, unsigned flags, int chunk, int input_cost,
                                                                     const gpmpc_input_constraints* ucons) {
    if ((input_cost || ucons) && (!m || m->action_dim < 1)) return 0;
    if (ucons && (ucons->n_rows < 1 || ucons->n_rows > GPMPC_MAX_CONS)) return 0;
    return gpmpc_linearised_fc_rollout_workspace_bytes(m, B, H, flags, chunk);
}

extern "C" int gpmpc_linearised_fc_rollout_inputs(const gpmpc_gp_model* m, int B, int H, const double* x0, const double* U, const double* K_dev,
                                                  size_t k_step_stride, const gpmpc_cost_params* cost, const gpmpc_state_constraints* cons,
                                                  unsigned flags, double* out_means, double* out_covs, double* out_jac, double* out_cost,
                                                  double* out_grad, double* out_g, double* out_gjac, int input_cost,
                                                  const gpmpc_input_constraints* ucons, double* out_gu, double* out_gujac, int chunk,
                                                  void* workspace, size_t workspace_bytes, void* stream) {
    const LpfInputs in = {input_cost, ucons, out_gu, out_gujac};
    return gpmpc_lpf_rollout("gpmpc_linearised_fc_rollout_inputs", m, B, H, x0, U, K_dev, k_step_stride, cost, cons, flags, out_means, out_covs,
                             out_jac, out_cost, out_grad, out_g, out_gjac, chunk, workspace, workspace_bytes, stream, &in);
}

// ---------------------------------------------------------------------------
// host: the particles' inputs
// ---------------------------------------------------------------------------
int gpmpc_lpi_particle_inputs(int B, int P, int ds, int da, const double* x_prev, const double* U_t, size_t u_stride, const double* K_t,
                              const double* mu_t, size_t mu_stride, double* out_u, hipStream_t s) {
    hipLaunchKernelGGL(k_lpi_pinputs, dim3(gpmpc_blocks256((long)B * P * da)), dim3(256), 0, s, B, P, ds, da, x_prev, U_t, u_stride, K_t, mu_t,
                       mu_stride, out_u);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

int gpmpc_lpi_assemble(int B, int P, int ds, int da, const double* x_prev, const double* U_p, const double* eps, const double* action_sd,
                       double* z, hipStream_t s) {
    LpiSd sd;
    memset(&sd, 0, sizeof(sd));
    memcpy(sd.v, action_sd, sizeof(double) * da);
    hipLaunchKernelGGL(k_lpi_assemble, dim3(gpmpc_blocks256((long)B * P * (ds + da))), dim3(256), 0, s, B, P, ds, da, x_prev, U_p, eps, sd, z);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

int gpmpc_lpi_input_stats(int B, int P, int H, int da, const double* inputs, const gpmpc_input_constraints* ucons, double* out_umean,
                          double* out_ucov, double* out_uviol, double* out_ujoint, hipStream_t s) {
    gpmpc_input_constraints cz;
    memset(&cz, 0, sizeof(cz));
    const int n_rows = ucons ? ucons->n_rows : 0;
    hipLaunchKernelGGL(k_lpi_ustats, dim3(H, B), dim3(MPPI_THREADS), 0, s, B, P, H, da, inputs, n_rows, ucons ? *ucons : cz, out_umean, out_ucov,
                       out_uviol);
    if (ucons) hipLaunchKernelGGL(k_lpi_ujoint, dim3(B), dim3(MPPI_THREADS), 0, s, B, P, H, da, inputs, n_rows, *ucons, out_ujoint);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

static int lpi_check_particles(const char* who, int B, int P, int da) {
    if (int rc = gpmpc_pt_check_bp(who, B, P)) return rc;
    if (da < 1 || da >= GPMPC_MAX_D) return gpmpc_refuse(who, "action_dim = %d outside 1...GPMPC_MAX_D - 1", da);
    return GPMPC_OK;
}

extern "C" int gpmpc_particle_inputs(int B, int P, int ds, int da, const double* x_prev, const double* U_t, size_t u_stride, const double* K_t,
                                     const double* mu_t, size_t mu_stride, double* out_u, void* stream) {
    const char* who = "gpmpc_particle_inputs";
    if (int rc = lpi_check_particles(who, B, P, da)) return rc;
    if (ds < 1 || ds > GPMPC_MAX_DS || ds + da > GPMPC_MAX_D) return gpmpc_refuse(who, "state_dim or action_dim outside the range");
    if (!x_prev || !U_t || !out_u) return gpmpc_refuse(who, "NULL pointer");
    if (K_t && !mu_t) return gpmpc_refuse(who, "a gain needs the mean trajectory it acts around (mu_t is NULL)");
    if (B > 1 && (u_stride < (size_t)da || (K_t && mu_stride < (size_t)ds))) return gpmpc_refuse(who, "u_stride < action_dim or mu_stride < state_dim");
    return gpmpc_lpi_particle_inputs(B, P, ds, da, x_prev, U_t, u_stride, K_t, mu_t, mu_stride, out_u, (hipStream_t)stream);
}

extern "C" int gpmpc_particle_input_stats(int B, int P, int H, int da, const double* inputs, const gpmpc_input_constraints* ucons,
                                          double* out_umean, double* out_ucov, double* out_uviol, double* out_ujoint, void* stream) {
    const char* who = "gpmpc_particle_input_stats";
    if (int rc = lpi_check_particles(who, B, P, da)) return rc;
    if (H < 1 || H > 65535) return gpmpc_refuse(who, "H (steps) outside 1...65535");
    if (B > 65535) return gpmpc_refuse(who, "B > 65535");
    if ((long)B * P * GPMPC_MAX_D * H > (1L << 40)) return gpmpc_refuse(who, "more than 2^40 input values");
    if (!inputs) return gpmpc_refuse(who, "NULL pointer");
    if (ucons) { if (int rc = gpmpc_lpi_check_rows(who, ucons)) return rc; }
    if ((ucons != nullptr) != (out_uviol != nullptr) || (ucons != nullptr) != (out_ujoint != nullptr))
        return gpmpc_refuse(who, "out_uviol and out_ujoint are given exactly when input rows are");
    return gpmpc_lpi_input_stats(B, P, H, da, inputs, ucons, out_umean, out_ucov, out_uviol, out_ujoint, (hipStream_t)stream);
}
