// Constrained multi-start on the device: an augmented Lagrangian over gpmpc_rollout_constrained with the lock-step L-BFGS of lbfgs.hip as
// the inner search (include/gpmpc.h).  Per start k: R = H n_rows constraint values g_i <= 0, multipliers lam_i >= 0,
// one penalty rho > 0.
//
//   k_al_merit    (cost, grad, g, g_jac, lam, rho) -> merit value M and gradient: what the tick kernel is fed instead of (cost, grad).
//   k_al_outer    one outer step of every start from the evaluation of its accepted point: incumbent, then (with `update`) the violation
//                 measure V, the multipliers, the penalty, the settled flag.
//   k_al_points   U <- X and a copy of X (the start step's X0 argument is __restrict__: it must not point into the state it writes).
//   k_al_init     the state a solve starts from.
//   k_al_finish   best = argmin of the incumbent keys, its plan, the count of alive starts that are not settled.
//
// k_al_merit follows k_rollout_constraints: grid (K, ceil(n / 64)), one wave per workgroup, lanes along the column c, so a row of g_jac is
// one coalesced read; g, lam and rho are read through wave-uniform addresses and every lane forms the same psi_i and the same merit sum --
// no LDS, no barrier, no atomics.  k_al_outer follows k_lbfgs_tick: one wave per start, per-lane maxima over i = lane, lane + 64, ... and
// the butterfly over the wave, branches on wave-uniform values only.  Every sum has a fixed order: a start's result depends neither on K
// nor on the grid.
#include "lbfgs_internal.h"
#include <cmath>

// offsets in doubles (include/gpmpc.h)
struct AlLayout { long sum, plan, rho, vprev, v, f, incv, incf, alive, settled, lam, incx, total; };

static AlLayout al_layout(int K, long n, long R) {
    AlLayout L;
    lbfgs_carver c;
    L.sum = c.take(32);
    L.plan = c.take(n);
    L.rho = c.take(K); L.vprev = c.take(K); L.v = c.take(K); L.f = c.take(K); L.incv = c.take(K); L.incf = c.take(K);
    L.alive = c.take(K); L.settled = c.take(K);
    L.lam = c.take(K * R);
    L.incx = c.take(K * n);
    L.total = c.total();
    return L;
}

__device__ __forceinline__ double al_wave_max(double v) {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v = fmax(v, __shfl_xor(v, h));
    return v;
}
__device__ __forceinline__ bool al_finite(double v) { return v - v == 0.0; }

// grid (K, ceil(n / 64)), one wave per workgroup
__global__ __launch_bounds__(64) void k_al_merit(int n, int R, const double* __restrict__ f, const double* __restrict__ grad,
                                                 const double* __restrict__ g, const double* __restrict__ gjac,
                                                 const double* __restrict__ lam, const double* __restrict__ rho, double* __restrict__ out_M,
                                                 double* __restrict__ out_grad) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const int c = blockIdx.y * 64 + lane;
    const bool live = c < n;
    const double* __restrict__ gk = g + (size_t)k * R;
    const double* __restrict__ lk = lam + (size_t)k * R;
    const double* __restrict__ Jk = gjac + (size_t)k * R * n;
    const double r = rho[k];
    double sum = 0.0, acc = 0.0;
    for (int i = 0; i < R; ++i) {
        const double l = lk[i];
        const double t = l + r * gk[i];
        // t <= 0: the row is inactive; NaN passes through (t > 0 and t <= 0 are both false for a NaN)
        const double psi = t > 0.0 ? t : (t <= 0.0 ? 0.0 : t);
        sum = sum + (psi * psi - l * l);
        if (psi != 0.0) {                                   // (wave-uniform) an inactive row of g_jac is not read
            if (live) acc = fma(psi, Jk[(size_t)i * n + c], acc);
        }
    }
    if (live) out_grad[(size_t)k * n + c] = grad[(size_t)k * n + c] + acc;
    if (blockIdx.y == 0 && lane == 0) out_M[k] = f[k] + (1.0 / (2.0 * r)) * sum;
}

// grid: K workgroups of one wave.  X [K][n]: the points (f, g) were evaluated at; conv [K] or NULL (= 0): the inner search's flags.
__global__ __launch_bounds__(64) void k_al_outer(int n, int R, gpmpc_auglag_params P, int update, AlLayout L, const double* __restrict__ f,
                                                 const double* __restrict__ g, const double* __restrict__ X,
                                                 const double* __restrict__ conv, double* st) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const double* __restrict__ gk = g + (size_t)k * R;
    double* lamk = st + L.lam + (size_t)k * R;
    const double fk = f[k];
    int fin = al_finite(fk) ? 1 : 0;
    double vm = 0.0;
    for (int i = lane; i < R; i += 64) {
        const double gi = gk[i];
        fin &= al_finite(gi) ? 1 : 0;
        vm = fmax(vm, gi > 0.0 ? gi : 0.0);
    }
    if (!__all(fin)) return;                                // (wave-uniform) a dead start: nothing of it is written
    const double v = al_wave_max(vm);
    const double kv = v <= P.feas_tol ? 0.0 : v;
    const double iv = st[L.incv + k], ic = st[L.incf + k];
    const bool better = kv < iv || (kv == iv && fk < ic);
    if (better) {                                           // (wave-uniform)
        const double* __restrict__ Xk = X + (size_t)k * n;
        double* inc = st + L.incx + (size_t)k * n;
        for (int c = lane; c < n; c += 64) inc[c] = Xk[c];
    }
    double rho = st[L.rho + k], V = 0.0;
    bool grow = false;
    if (update) {                                           // (wave-uniform)
        double Vm = 0.0;
        for (int i = lane; i < R; i += 64) {
            const double l = lamk[i], gi = gk[i];
            const double lo = -l / rho;
            Vm = fmax(Vm, fabs(gi > lo ? gi : lo));
            double t = l + rho * gi;
            t = t > 0.0 ? t : 0.0;
            lamk[i] = t > P.lam_max ? P.lam_max : t;
        }
        V = al_wave_max(Vm);
        grow = V > P.shrink * st[L.vprev + k];
        if (grow) {
            rho = P.growth * rho;
            rho = rho > P.rho_max ? P.rho_max : rho;
        }
    }
    if (lane == 0) {
        st[L.v + k] = v;
        st[L.f + k] = fk;
        if (better) { st[L.incv + k] = kv; st[L.incf + k] = fk; }
        if (update) {
            st[L.rho + k] = rho;
            st[L.vprev + k] = V;
            st[L.settled + k] = (V <= P.feas_tol && conv && conv[k] != 0.0) ? 1.0 : 0.0;
        }
    }
}

// grid: K workgroups of one wave
__global__ __launch_bounds__(64) void k_al_points(int n, const double* __restrict__ X, double* __restrict__ U, double* __restrict__ copy) {
    const size_t o = (size_t)blockIdx.x * n;
    for (int c = threadIdx.x; c < n; c += 64) {
        const double x = X[o + c];
        U[o + c] = x;
        copy[o + c] = x;
    }
}

// grid: K workgroups of one wave
__global__ __launch_bounds__(64) void k_al_init(int n, int da, int R, gpmpc_auglag_params P, AlLayout L, const double* __restrict__ X0,
                                                double* __restrict__ st) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const double* X0k = X0 + (size_t)k * n;
    double* inc = st + L.incx + (size_t)k * n;
    double* lamk = st + L.lam + (size_t)k * R;
    for (int c = lane; c < n; c += 64) {
        const int j = c % da;
        double x = X0k[c];
        x = x < P.inner.lb[j] ? P.inner.lb[j] : x;
        inc[c] = x > P.inner.ub[j] ? P.inner.ub[j] : x;
    }
    for (int i = lane; i < R; i += 64) lamk[i] = 0.0;
    if (lane == 0) {
        const double inf = __builtin_huge_val();
        st[L.rho + k] = P.rho0;
        st[L.vprev + k] = inf;
        st[L.v + k] = inf;
        st[L.f + k] = inf;
        st[L.incv + k] = inf;
        st[L.incf + k] = inf;
        st[L.alive + k] = 1.0;
        st[L.settled + k] = 0.0;
    }
}

// grid: one workgroup of 256 threads (K <= 256).  alive_in [K] or NULL: the inner search's alive flags become the state's.
__global__ __launch_bounds__(256) void k_al_finish(int K, int n, int R, AlLayout L, const double* __restrict__ alive_in, double* st) {
    __shared__ double kv[256], kf[256];
    __shared__ int ki[256], open[256];
    const int t = threadIdx.x;
    const double inf = __builtin_huge_val();
    double alive = 0.0;
    if (t < K) {
        alive = alive_in ? alive_in[t] : st[L.alive + t];
        if (alive_in) st[L.alive + t] = alive;
    }
    kv[t] = t < K ? st[L.incv + t] : inf;
    kf[t] = t < K ? st[L.incf + t] : inf;
    ki[t] = t < K ? t : 0x7fffffff;
    open[t] = (t < K && alive != 0.0 && st[L.settled + t] == 0.0) ? 1 : 0;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) {
            const double v2 = kv[t + h], f2 = kf[t + h];
            const int i2 = ki[t + h];
            const bool less = v2 < kv[t] || (v2 == kv[t] && (f2 < kf[t] || (f2 == kf[t] && i2 < ki[t])));
            if (less) { kv[t] = v2; kf[t] = f2; ki[t] = i2; }
            open[t] += open[t + h];
        }
        __syncthreads();
    }
    const int best = ki[0];                                 // every key (+inf, +inf): the lowest index is row 0
    const double* X = st + L.incx + (size_t)best * n;
    for (int c = t; c < n; c += 256) st[L.plan + c] = X[c];
    if (t < 32) {
        double v = 0.0;
        if (t == 0) v = (double)open[0];
        if (t == 1) v = (double)best;
        if (t == 2) v = kv[0];
        if (t == 3) v = kf[0];
        if (t == 4) v = (double)K;
        if (t == 5) v = (double)n;
        if (t == 6) v = (double)R;
        st[L.sum + t] = v;
    }
}

// ---------------------------------------------------------------------------
// host entries
// ---------------------------------------------------------------------------
static int al_check_scalars(const gpmpc_auglag_params* P, const char* who) {
    if (!P) return GPMPC_E_ARG;
    if (int rc = lbfgs_check_scalars(&P->inner, who)) return rc;
    const double pos[3] = {P->rho0, P->growth, P->rho_max};
    const char* pos_name[3] = {"rho0", "growth", "rho_max"};
    for (int i = 0; i < 3; ++i)
        if (!(pos[i] > 0.0)) return gpmpc_refuse(who, "%s = %g is not positive", pos_name[i], pos[i]);
    if (!(P->growth >= 1.0)) return gpmpc_refuse(who, "growth = %g is less than 1", P->growth);
    if (!(P->shrink > 0.0 && P->shrink <= 1.0)) return gpmpc_refuse(who, "shrink = %g outside (0, 1]", P->shrink);
    const double nn[2] = {P->feas_tol, P->lam_max};
    const char* nn_name[2] = {"feas_tol", "lam_max"};
    for (int i = 0; i < 2; ++i)
        if (!(nn[i] >= 0.0)) return gpmpc_refuse(who, "%s = %g is negative or NaN", nn_name[i], nn[i]);
    if (P->inner_ticks < 1) return gpmpc_refuse(who, "inner_ticks = %d is less than 1", P->inner_ticks);
    return GPMPC_OK;
}

static int al_rows_ok(int n_rows) { return n_rows >= 1 && n_rows <= GPMPC_MAX_CONS; }

extern "C" size_t gpmpc_auglag_state_bytes(int K, int H, int da, int n_rows) {
    if (K < 1 || K > GPMPC_LBFGS_MAX_STARTS || !al_rows_ok(n_rows) || !gpmpc_solver_dims_ok(H, 0, da)) return 0;
    return sizeof(double) * (size_t)al_layout(K, (long)H * da, (long)H * n_rows).total;
}

static int al_launch_merit(int K, int n, int R, const double* f, const double* grad, const double* g, const double* gjac, const double* lam,
                           const double* rho, double* out_M, double* out_grad, hipStream_t s) {
    hipLaunchKernelGGL(k_al_merit, dim3(K, (n + 63) / 64), dim3(64), 0, s, n, R, f, grad, g, gjac, lam, rho, out_M, out_grad);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}
static int al_launch_outer(int n, int R, const gpmpc_auglag_params& P, int update, const AlLayout& L, const double* f, const double* g,
                           const double* X, const double* conv, double* st, hipStream_t s) {
    hipLaunchKernelGGL(k_al_outer, dim3(P.inner.n_starts), dim3(64), 0, s, n, R, P, update, L, f, g, X, conv, st);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}
static int al_launch_finish(int K, int n, int R, const AlLayout& L, const double* alive, double* st, hipStream_t s) {
    hipLaunchKernelGGL(k_al_finish, dim3(1), dim3(256), 0, s, K, n, R, L, alive, st);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

extern "C" int gpmpc_auglag_merit(int K, int H, int da, int n_rows, const double* f, const double* grad, const double* g, const double* gjac,
                                  const double* lam, const double* rho, double* out_M, double* out_grad, void* stream) {
    if (!f || !grad || !g || !gjac || !lam || !rho || !out_M || !out_grad || K < 1 || !al_rows_ok(n_rows) || !gpmpc_solver_dims_ok(H, 0, da))
        return GPMPC_E_ARG;
    return al_launch_merit(K, H * da, H * n_rows, f, grad, g, gjac, lam, rho, out_M, out_grad, (hipStream_t)stream);
}

extern "C" int gpmpc_auglag_outer(int H, int da, int n_rows, const gpmpc_auglag_params* P, int update, const double* f, const double* g,
                                  const double* X, const double* conv, const double* alive, void* state, size_t state_bytes, void* stream) {
    const char* who = "gpmpc_auglag_outer";
    if (!P || !f || !g || !X || !state || !al_rows_ok(n_rows) || !gpmpc_solver_dims_ok(H, 0, da)) return GPMPC_E_ARG;
    if (int rc = al_check_scalars(P, who)) return rc;
    const int K = P->inner.n_starts, n = H * da, R = H * n_rows;
    const AlLayout L = al_layout(K, n, R);
    if (state_bytes < sizeof(double) * (size_t)L.total) return GPMPC_E_WORKSPACE;
    if (int rc = al_launch_outer(n, R, *P, update != 0, L, f, g, X, conv, (double*)state, (hipStream_t)stream)) return rc;
    return al_launch_finish(K, n, R, L, alive, (double*)state, (hipStream_t)stream);
}

// workspace of a solve: state | the inner search's state | x0 [K][ds] | cost [K] | grad [K][n] | g [K][R] | g_jac [K][R][n] | M [K] |
// merit gradient [K][n] | copy of X [K][n] | the rollout's own workspace
struct AlWorkspace { size_t off_lb, off_x0, off_cost, off_grad, off_g, off_gjac, off_M, off_gM, off_copy, off_roll, total; gpmpc_solver_eval_layout roll; };
static AlWorkspace al_workspace(const gpmpc_pack* p, int H, int K, int n_rows, const AlLayout& L, const LbfgsLayout& LB, gpmpc_solver_rule rule) {
    AlWorkspace W;
    const size_t n = (size_t)H * p->da, R = (size_t)H * n_rows, d = sizeof(double);
    gpmpc_carver c;
    c.take(d * (size_t)L.total);
    W.off_lb = c.take(d * (size_t)LB.total);
    W.off_x0 = c.take(d * K * p->ds);
    W.off_cost = c.take(d * K);
    W.off_grad = c.take(d * K * n);
    W.off_g = c.take(d * K * R);
    W.off_gjac = c.take(d * K * R * n);
    W.off_M = c.take(d * K);
    W.off_gM = c.take(d * K * n);
    W.off_copy = c.take(d * K * n);
    W.roll = gpmpc_solver_eval_bytes(rule, p, K, H, true, GPMPC_WANT_GRAD);
    W.off_roll = c.take(W.roll.total);
    W.total = c.total();
    return W;
}

static size_t al_solve_bytes(gpmpc_solver_rule rule, const gpmpc_pack* p, int H, const gpmpc_state_constraints* cons, const gpmpc_auglag_params* P) {
    if (!p || !P || !cons || !al_rows_ok(cons->n_rows)) return 0;
    const int K = P->inner.n_starts, m = P->inner.history;
    if (K < 1 || K > GPMPC_LBFGS_MAX_STARTS || m < 1 || m > GPMPC_LBFGS_MAX_HISTORY || !gpmpc_solver_dims_ok(H, p->ds, p->da)) return 0;
    const long n = (long)H * p->da;
    return al_workspace(p, H, K, cons->n_rows, al_layout(K, n, (long)H * cons->n_rows), lbfgs_layout(K, n, m), rule).total;
}
extern "C" size_t gpmpc_auglag_solve_workspace_bytes(const gpmpc_pack* p, int H, const gpmpc_state_constraints* cons,
                                                     const gpmpc_auglag_params* P) {
    return al_solve_bytes(GPMPC_RULE_DIAGONAL, p, H, cons, P);
}
extern "C" size_t gpmpc_auglag_solve_fullcov_workspace_bytes(const gpmpc_pack* p, int H, const gpmpc_state_constraints* cons,
                                                             const gpmpc_auglag_params* P) {
    return al_solve_bytes(GPMPC_RULE_FULLCOV, p, H, cons, P);
}

// the solve of both entries; the rule decides the one evaluation (solver_frame.h)
static int al_solve(gpmpc_solver_rule rule, const char* who, const gpmpc_pack* p, int H, const double* x0, const double* X0,
                    const gpmpc_cost_params* cost, const gpmpc_state_constraints* cons, const gpmpc_auglag_params* P, int first_outer,
                    int n_outer, void* workspace, size_t workspace_bytes, void* stream) {
    if (!p || !x0 || !cost || !cons || !P || !workspace || H < 1 || (first_outer == 0 && !X0)) return GPMPC_E_ARG;
    if (int rc = al_check_scalars(P, who)) return rc;                    // (before the pack is looked at)
    if (first_outer < 0) return gpmpc_refuse(who, "first_outer is negative");
    if (n_outer < 0) return gpmpc_refuse(who, "n_outer is negative");
    if (int rc = gpmpc_solver_enter(p, H, cost, cons, who, [&](int da) { return gpmpc_check_bounds(P->inner.lb, P->inner.ub, da, who); }, rule))
        return rc;
    const gpmpc_lbfgs_params& PI = P->inner;
    const int K = PI.n_starts, n = H * p->da, R = H * cons->n_rows, ds = p->ds, da = p->da;
    const AlLayout L = al_layout(K, n, R);
    const LbfgsLayout LB = lbfgs_layout(K, n, PI.history);
    const AlWorkspace W = al_workspace(p, H, K, cons->n_rows, L, LB, rule);
    if (workspace_bytes < W.total) return GPMPC_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    double *st = (double*)ws, *lb = (double*)(ws + W.off_lb), *x0b = (double*)(ws + W.off_x0), *cst = (double*)(ws + W.off_cost);
    double *grd = (double*)(ws + W.off_grad), *g = (double*)(ws + W.off_g), *gjac = (double*)(ws + W.off_gjac);
    double *M = (double*)(ws + W.off_M), *gM = (double*)(ws + W.off_gM), *copy = (double*)(ws + W.off_copy);
    double *U = lb + LB.U, *X = lb + LB.X;
    auto evaluate = [&]() {
        return gpmpc_solver_eval(rule, p, K, H, x0b, U, cost, cons, GPMPC_WANT_GRAD, cst, grd, g, gjac, ws + W.off_roll, W.roll, stream);
    };
    auto merit = [&]() { return al_launch_merit(K, n, R, cst, grd, g, gjac, st + L.lam, st + L.rho, M, gM, s); };
    if (first_outer == 0) {
        hipLaunchKernelGGL(k_al_init, dim3(K), dim3(64), 0, s, n, da, R, *P, L, X0, st);
        GPMPC_HIP(hipGetLastError());
        if (int rc = lbfgs_launch_start(n, ds, da, PI, LB, X0, nullptr, nullptr, x0, x0b, lb, s)) return rc;      // U = clip(X0)
    }
    for (int o = first_outer; o < first_outer + n_outer; ++o) {
        if (o > 0) {
            hipLaunchKernelGGL(k_al_points, dim3(K), dim3(64), 0, s, n, X, U, copy);
            GPMPC_HIP(hipGetLastError());
        }
        if (int rc = evaluate()) return rc;
        if (int rc = al_launch_outer(n, R, *P, o > 0, L, cst, g, U, lb + LB.conv, st, s)) return rc;
        if (int rc = merit()) return rc;
        if (int rc = lbfgs_launch_start(n, ds, da, PI, LB, o > 0 ? copy : X0, M, gM, nullptr, nullptr, lb, s)) return rc;
        for (int t = 0; t < P->inner_ticks; ++t) {
            if (int rc = evaluate()) return rc;
            if (int rc = merit()) return rc;
            if (int rc = lbfgs_launch_tick(n, da, PI, LB, M, gM, lb, s)) return rc;
        }
    }
    const bool searched = first_outer + n_outer > 0;        // (an inner search has run in this workspace: X and its flags exist)
    if (searched) {
        hipLaunchKernelGGL(k_al_points, dim3(K), dim3(64), 0, s, n, X, U, copy);
        GPMPC_HIP(hipGetLastError());
    }
    if (int rc = evaluate()) return rc;
    if (int rc = al_launch_outer(n, R, *P, 0, L, cst, g, U, nullptr, st, s)) return rc;
    if (searched)
        if (int rc = lbfgs_launch_finish(n, PI, LB, lb, s)) return rc;
    return al_launch_finish(K, n, R, L, searched ? lb + LB.alive : nullptr, st, s);
}

extern "C" int gpmpc_auglag_solve(const gpmpc_pack* p, int H, const double* x0, const double* X0, const gpmpc_cost_params* cost,
                                  const gpmpc_state_constraints* cons, const gpmpc_auglag_params* P, int first_outer, int n_outer,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    return al_solve(GPMPC_RULE_DIAGONAL, "gpmpc_auglag_solve", p, H, x0, X0, cost, cons, P, first_outer, n_outer, workspace, workspace_bytes,
                    stream);
}

extern "C" int gpmpc_auglag_solve_fullcov(const gpmpc_pack* p, int H, const double* x0, const double* X0, const gpmpc_cost_params* cost,
                                          const gpmpc_state_constraints* cons, const gpmpc_auglag_params* P, int first_outer, int n_outer,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    return al_solve(GPMPC_RULE_FULLCOV, "gpmpc_auglag_solve_fullcov", p, H, x0, X0, cost, cons, P, first_outer, n_outer, workspace,
                    workspace_bytes, stream);
}
