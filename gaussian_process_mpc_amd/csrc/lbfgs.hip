// Lock-step multi-start L-BFGS on the device (include/gpmpc.h): K bounded quasi-Newton searches advanced together, one
// batched evaluation (a B = K rollout with gradient) per tick.  The rule is that of multistart.lockstep_lbfgs (line_points = 1, no patience).
//
//   k_lbfgs_start   phase 0 (no evaluation given): U = clip(X0) and the start state repeated K times -- the batch the start evaluation runs on.
//                   phase 1: X, F, G from that evaluation, the first direction (steepest descent on the free components), the first trial point.
//   k_lbfgs_tick    one step of every start's state machine from the evaluation of its trial point: Armijo test, then accept (store the pair,
//                   move, two-loop recursion for the new direction) or halve the step; writes the next trial point into U.
//   k_lbfgs_finish  best = argmin F, its plan, the count of starts not done.
//
// One workgroup of ONE wave per start, lanes along c = lane, lane + 64, ...  A lane only ever reads back vector elements it wrote itself
// (q, D, X, G, S, Y are all indexed by the lane's own c), scalars live in registers of every lane: no barrier, no cross-lane traffic through
// memory.  Every dot product: the lane's partial sum over its c in ascending order, then a butterfly over the wave (partner lane ^ 32, ^ 16,
// ... ^ 1; a + b is commutative, so every lane holds the same bits).  No atomics: a start's result does not depend on K or the grid.
// Branches are taken on wave-uniform values only (the reductions' results); a rejected trial point never reaches X, G or the pairs.
#include "lbfgs_internal.h"
#include <cmath>

#define LBFGS_Q_LDS 2048                // the two-loop vector q lives in LDS up to this n, in the D row of the state (global) beyond
// (LbfgsLayout, the offsets of the state's fields, is in lbfgs_internal.h: auglag.hip runs its inner search through the launches below)

__device__ __forceinline__ double lbfgs_wave_sum(double v) {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v = v + __shfl_xor(v, h);
    return v;
}
__device__ __forceinline__ double lbfgs_wave_max(double v) {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v = fmax(v, __shfl_xor(v, h));
    return v;
}
__device__ __forceinline__ bool lbfgs_finite(double v) { return v - v == 0.0; }
__device__ __forceinline__ double lbfgs_clip(double v, double lo, double hi) {
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}
// a component the gradient pins at a bound
__device__ __forceinline__ bool lbfgs_pinned(double x, double g, double lo, double hi) { return (x <= lo && g > 0.0) || (x >= hi && g < 0.0); }

// The new direction of one start from its (X, G) and the cnt pairs in the ring (newest in slot head): writes D, returns the first step
// length; pg = max |g_free|.  A direction that is not a descent direction, or not finite, is replaced by -g_free and drops the pairs.
// q: n doubles of which lane l uses the elements l, l + 64, ... (may be the D row itself).
__device__ __forceinline__ double lbfgs_direction(int n, int da, int m, const gpmpc_lbfgs_params& P, const double* X, const double* G, double* D,
                                                  const double* S, const double* Y, const double* rho, int& cnt, int head, double* q,
                                                  double* alpha, double& pg) {
    const int lane = threadIdx.x;
    double gg = 0.0, pm = 0.0;
    for (int c = lane; c < n; c += 64) {
        const int j = c % da;
        const double g = G[c];
        const double gf = lbfgs_pinned(X[c], g, P.lb[j], P.ub[j]) ? 0.0 : g;
        q[c] = gf;
        gg = gg + gf * gf;
        pm = fmax(pm, fabs(gf));
    }
    gg = lbfgs_wave_sum(gg);
    pg = lbfgs_wave_max(pm);
    for (int j = 0; j < cnt; ++j) {                         // newest pair first
        const int slot = (head + j) % m;
        const double *Sj = S + (size_t)slot * n, *Yj = Y + (size_t)slot * n;
        double d = 0.0;
        for (int c = lane; c < n; c += 64) d = d + Sj[c] * q[c];
        const double a = rho[slot] * lbfgs_wave_sum(d);
        alpha[j] = a;
        for (int c = lane; c < n; c += 64) q[c] = q[c] - a * Yj[c];
    }
    if (cnt > 0) {                                          // gamma = s.y / y.y of the newest pair
        const double* Y0 = Y + (size_t)head * n;
        double d = 0.0;
        for (int c = lane; c < n; c += 64) d = d + Y0[c] * Y0[c];
        const double yy = lbfgs_wave_sum(d);
        if (yy > 0.0) {
            const double inv = 1.0 / (rho[head] * yy);
            for (int c = lane; c < n; c += 64) q[c] = q[c] * inv;
        }
    }
    for (int j = cnt - 1; j >= 0; --j) {                    // oldest pair first
        const int slot = (head + j) % m;
        const double *Sj = S + (size_t)slot * n, *Yj = Y + (size_t)slot * n;
        double d = 0.0;
        for (int c = lane; c < n; c += 64) d = d + Yj[c] * q[c];
        const double coef = alpha[j] - rho[slot] * lbfgs_wave_sum(d);
        for (int c = lane; c < n; c += 64) q[c] = q[c] + coef * Sj[c];
    }
    double sl = 0.0;
    int fin = 1;
    for (int c = lane; c < n; c += 64) {
        const int j = c % da;
        const double g = G[c];
        const bool pin = lbfgs_pinned(X[c], g, P.lb[j], P.ub[j]);
        const double gf = pin ? 0.0 : g, d = pin ? 0.0 : -q[c];
        D[c] = d;
        sl = sl + d * gf;
        fin &= lbfgs_finite(d) ? 1 : 0;
    }
    const double slope = lbfgs_wave_sum(sl);
    if (!(slope < 0.0) || !__all(fin)) {                    // (wave-uniform)
        for (int c = lane; c < n; c += 64) {
            const int j = c % da;
            const double g = G[c];
            D[c] = -(lbfgs_pinned(X[c], g, P.lb[j], P.ub[j]) ? 0.0 : g);
        }
        cnt = 0;
    }
    const double gn = sqrt(gg);
    return cnt == 0 ? fmin(1.0, 1.0 / (gn > 0.0 ? gn : 1.0)) : 1.0;
}

// U = clip(X + A D), or X for a done start
__device__ __forceinline__ void lbfgs_trial(int n, int da, const gpmpc_lbfgs_params& P, const double* X, const double* D, double A, bool done,
                                            double* U) {
    for (int c = threadIdx.x; c < n; c += 64) {
        const int j = c % da;
        const double x = X[c];
        U[c] = done ? x : lbfgs_clip(x + A * D[c], P.lb[j], P.ub[j]);
    }
}

// grid: K workgroups of one wave.  cost == NULL: phase 0.
__global__ __launch_bounds__(64) void k_lbfgs_start(int n, int da, int ds, gpmpc_lbfgs_params P, LbfgsLayout L, const double* __restrict__ X0,
                                                    const double* __restrict__ cost, const double* __restrict__ grad,
                                                    const double* __restrict__ x0, double* __restrict__ x0b, double* st) {
    __shared__ double qs[LBFGS_Q_LDS];
    __shared__ double alpha[GPMPC_LBFGS_MAX_HISTORY];
    const int k = blockIdx.x, lane = threadIdx.x, m = P.history;
    const double* X0k = X0 + (size_t)k * n;
    double* U = st + L.U + (size_t)k * n;
    if (x0b && lane < ds) x0b[(size_t)k * ds + lane] = x0[lane];
    if (!cost) {
        for (int c = lane; c < n; c += 64) { const int j = c % da; U[c] = lbfgs_clip(X0k[c], P.lb[j], P.ub[j]); }
        return;
    }
    const double* gk = grad + (size_t)k * n;
    double *X = st + L.X + (size_t)k * n, *G = st + L.G + (size_t)k * n, *D = st + L.D + (size_t)k * n;
    double *S = st + L.S + (size_t)k * n * m, *Y = st + L.Y + (size_t)k * n * m, *rho = st + L.rho + (size_t)k * m;
    const double f = cost[k];
    int fin = 1;
    for (int c = lane; c < n; c += 64) fin &= lbfgs_finite(gk[c]) ? 1 : 0;
    const bool alive = lbfgs_finite(f) && __all(fin);
    for (int c = lane; c < n; c += 64) {
        const int j = c % da;
        X[c] = lbfgs_clip(X0k[c], P.lb[j], P.ub[j]);
        G[c] = alive ? gk[c] : 0.0;
    }
    for (size_t e = lane; e < (size_t)n * m; e += 64) { S[e] = 0.0; Y[e] = 0.0; }
    if (lane < m) rho[lane] = 0.0;
    int cnt = 0;
    double pg;
    const double a0 = lbfgs_direction(n, da, m, P, X, G, D, S, Y, rho, cnt, 0, n <= LBFGS_Q_LDS ? qs : D, alpha, pg);
    const bool done = !alive || pg <= P.gtol;
    if (lane == 0) {
        st[L.F + k] = alive ? f : __builtin_huge_val();
        st[L.conv + k] = (done && alive) ? 1.0 : 0.0;
        st[L.alive + k] = alive ? 1.0 : 0.0;
        st[L.iters + k] = 0.0;
        st[L.ticks + k] = 0.0;
        st[L.done + k] = done ? 1.0 : 0.0;
        st[L.A + k] = a0;
        st[L.cnt + k] = 0.0;
        st[L.head + k] = 0.0;
    }
    lbfgs_trial(n, da, P, X, D, a0, done, U);
}

// grid: K workgroups of one wave
__global__ __launch_bounds__(64) void k_lbfgs_tick(int n, int da, gpmpc_lbfgs_params P, LbfgsLayout L, const double* __restrict__ cost,
                                                   const double* __restrict__ grad, double* st) {
    __shared__ double qs[LBFGS_Q_LDS];
    __shared__ double alpha[GPMPC_LBFGS_MAX_HISTORY];
    const int k = blockIdx.x, lane = threadIdx.x, m = P.history;
    if (st[L.done + k] != 0.0) return;                      // a done start: evaluated at X, ignored, its state left as it is
    const double* gt = grad + (size_t)k * n;
    double *X = st + L.X + (size_t)k * n, *G = st + L.G + (size_t)k * n, *D = st + L.D + (size_t)k * n, *U = st + L.U + (size_t)k * n;
    double *S = st + L.S + (size_t)k * n * m, *Y = st + L.Y + (size_t)k * n * m, *rho = st + L.rho + (size_t)k * m;
    double F = st[L.F + k], A = st[L.A + k];
    int cnt = (int)st[L.cnt + k], head = (int)st[L.head + k];
    const double ft = cost[k];

    // Armijo test of the trial point
    double gs = 0.0;
    int fin = 1;
    for (int c = lane; c < n; c += 64) {
        fin &= lbfgs_finite(gt[c]) ? 1 : 0;
        gs = gs + G[c] * (U[c] - X[c]);
    }
    gs = lbfgs_wave_sum(gs);
    const bool ok = lbfgs_finite(ft) && __all(fin) && ft <= F + P.c1 * gs;
    bool done = false;
    if (ok) {                                               // (wave-uniform) accept
        double sy = 0.0, ss = 0.0, yy = 0.0;
        for (int c = lane; c < n; c += 64) {
            const double s = U[c] - X[c], y = gt[c] - G[c];
            sy = sy + s * y;
            ss = ss + s * s;
            yy = yy + y * y;
        }
        sy = lbfgs_wave_sum(sy); ss = lbfgs_wave_sum(ss); yy = lbfgs_wave_sum(yy);
        const bool keep = sy > 1e-10 * sqrt(ss * yy);
        if (keep) {
            head = (head + m - 1) % m;
            cnt = cnt + 1 < m ? cnt + 1 : m;
            rho[head] = 1.0 / sy;                           // (every lane writes the same value: each reads back its own store)
        }
        double *Sn = S + (size_t)head * n, *Yn = Y + (size_t)head * n;
        for (int c = lane; c < n; c += 64) {
            const double xt = U[c], g = gt[c];
            if (keep) { Sn[c] = xt - X[c]; Yn[c] = g - G[c]; }
            X[c] = xt;
            G[c] = g;
        }
        const double small_rhs = P.ftol * fmax(fmax(fabs(F), fabs(ft)), 1.0);
        const bool small = (F - ft) <= small_rhs;
        F = ft;
        double pg;
        A = lbfgs_direction(n, da, m, P, X, G, D, S, Y, rho, cnt, head, n <= LBFGS_Q_LDS ? qs : D, alpha, pg);
        done = small || pg <= P.gtol;
        if (lane == 0) {
            st[L.F + k] = F;
            st[L.iters + k] = st[L.iters + k] + 1.0;
            st[L.cnt + k] = (double)cnt;
            st[L.head + k] = (double)head;
        }
    } else {                                                // shrink
        A = A * 0.5;
        double dm = 0.0;
        for (int c = lane; c < n; c += 64) dm = fmax(dm, fabs(D[c]));
        dm = lbfgs_wave_max(dm);
        done = A * dm < P.min_step;                         // no representable descent step left
    }
    if (lane == 0) {
        st[L.A + k] = A;
        st[L.ticks + k] = st[L.ticks + k] + 1.0;
        if (done) { st[L.done + k] = 1.0; st[L.conv + k] = 1.0; }
    }
    lbfgs_trial(n, da, P, X, D, A, done, U);
}

// grid: one workgroup of 256 threads (K <= 256)
__global__ __launch_bounds__(256) void k_lbfgs_finish(int K, int n, int m, LbfgsLayout L, double* st) {
    __shared__ double fv[256];
    __shared__ int fi[256], nd[256];
    const int t = threadIdx.x;
    fv[t] = t < K ? st[L.F + t] : __builtin_huge_val();
    fi[t] = t < K ? t : 0x7fffffff;
    nd[t] = (t < K && st[L.done + t] == 0.0) ? 1 : 0;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) {
            const double f2 = fv[t + h];
            const int i2 = fi[t + h];
            if (f2 < fv[t] || (f2 == fv[t] && i2 < fi[t])) { fv[t] = f2; fi[t] = i2; }
            nd[t] += nd[t + h];
        }
        __syncthreads();
    }
    const int best = fi[0];                                 // no finite F: every F is +inf, the lowest index is row 0
    const double* X = st + L.X + (size_t)best * n;
    for (int c = t; c < n; c += 256) st[L.plan + c] = X[c];
    if (t < 32) {
        double v = 0.0;
        if (t == 0) v = (double)nd[0];
        if (t == 1) v = (double)best;
        if (t == 2) v = fv[0];
        if (t == 3) v = (double)K;
        if (t == 4) v = (double)n;
        if (t == 5) v = (double)m;
        st[L.sum + t] = v;
    }
}

// ---------------------------------------------------------------------------
// host entries
// ---------------------------------------------------------------------------
// the part of the parameters that needs no dimension
int lbfgs_check_scalars(const gpmpc_lbfgs_params* P, const char* who) {
    if (!P) return GPMPC_E_ARG;
    if (P->n_starts < 1 || P->n_starts > GPMPC_LBFGS_MAX_STARTS)
        return gpmpc_refuse(who, "n_starts = %d outside 1..%d", P->n_starts, GPMPC_LBFGS_MAX_STARTS);
    if (P->history < 1 || P->history > GPMPC_LBFGS_MAX_HISTORY)
        return gpmpc_refuse(who, "history = %d outside 1..%d", P->history, GPMPC_LBFGS_MAX_HISTORY);
    const double v[4] = {P->gtol, P->ftol, P->c1, P->min_step};
    const char* name[4] = {"gtol", "ftol", "c1", "min_step"};
    for (int i = 0; i < 4; ++i)
        if (!(v[i] >= 0.0)) return gpmpc_refuse(who, "%s = %g is negative or NaN", name[i], v[i]);
    return GPMPC_OK;
}

extern "C" size_t gpmpc_lbfgs_state_bytes(int K, int H, int da, int m) {
    if (K < 1 || K > GPMPC_LBFGS_MAX_STARTS || m < 1 || m > GPMPC_LBFGS_MAX_HISTORY || !gpmpc_solver_dims_ok(H, 0, da)) return 0;
    return sizeof(double) * (size_t)lbfgs_layout(K, (long)H * da, m).total;
}

int lbfgs_launch_finish(int n, const gpmpc_lbfgs_params& P, const LbfgsLayout& L, double* st, hipStream_t s) {
    hipLaunchKernelGGL(k_lbfgs_finish, dim3(1), dim3(256), 0, s, P.n_starts, n, P.history, L, st);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}
int lbfgs_launch_start(int n, int ds, int da, const gpmpc_lbfgs_params& P, const LbfgsLayout& L, const double* X0, const double* cost,
                              const double* grad, const double* x0, double* x0b, double* st, hipStream_t s) {
    hipLaunchKernelGGL(k_lbfgs_start, dim3(P.n_starts), dim3(64), 0, s, n, da, ds, P, L, X0, cost, grad, x0, x0b, st);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}
int lbfgs_launch_tick(int n, int da, const gpmpc_lbfgs_params& P, const LbfgsLayout& L, const double* cost, const double* grad,
                             double* st, hipStream_t s) {
    hipLaunchKernelGGL(k_lbfgs_tick, dim3(P.n_starts), dim3(64), 0, s, n, da, P, L, cost, grad, st);
    GPMPC_HIP(hipGetLastError());
    return GPMPC_OK;
}

extern "C" int gpmpc_lbfgs_start(int H, int ds, int da, const gpmpc_lbfgs_params* P, const double* X0, const double* cost, const double* grad,
                                 const double* x0, double* out_x0_batch, void* state, size_t state_bytes, void* stream) {
    const char* who = "gpmpc_lbfgs_start";
    if (!P || !X0 || !state || (cost != nullptr) != (grad != nullptr) || !gpmpc_solver_dims_ok(H, ds, da) || (out_x0_batch && (!x0 || ds < 1)))
        return GPMPC_E_ARG;
    if (int rc = lbfgs_check_scalars(P, who)) return rc;
    if (int rc = gpmpc_check_bounds(P->lb, P->ub, da, who)) return rc;
    const int n = H * da;
    const LbfgsLayout L = lbfgs_layout(P->n_starts, n, P->history);
    if (state_bytes < sizeof(double) * (size_t)L.total) return GPMPC_E_WORKSPACE;
    if (int rc = lbfgs_launch_start(n, ds, da, *P, L, X0, cost, grad, x0, out_x0_batch, (double*)state, (hipStream_t)stream)) return rc;
    return cost ? lbfgs_launch_finish(n, *P, L, (double*)state, (hipStream_t)stream) : GPMPC_OK;
}

extern "C" int gpmpc_lbfgs_tick(int H, int da, const gpmpc_lbfgs_params* P, const double* cost, const double* grad, void* state,
                                size_t state_bytes, void* stream) {
    const char* who = "gpmpc_lbfgs_tick";
    if (!P || !cost || !grad || !state || !gpmpc_solver_dims_ok(H, 0, da)) return GPMPC_E_ARG;
    if (int rc = lbfgs_check_scalars(P, who)) return rc;
    if (int rc = gpmpc_check_bounds(P->lb, P->ub, da, who)) return rc;
    const int n = H * da;
    const LbfgsLayout L = lbfgs_layout(P->n_starts, n, P->history);
    if (state_bytes < sizeof(double) * (size_t)L.total) return GPMPC_E_WORKSPACE;
    if (int rc = lbfgs_launch_tick(n, da, *P, L, cost, grad, (double*)state, (hipStream_t)stream)) return rc;
    return lbfgs_launch_finish(n, *P, L, (double*)state, (hipStream_t)stream);
}

// workspace of a solve: state | x0 [K][ds] | cost [K] | grad [K][n] | the rollout's own workspace
struct LbfgsWorkspace { size_t off_x0, off_cost, off_grad, off_roll, total; gpmpc_solver_eval_layout roll; };
static LbfgsWorkspace lbfgs_workspace(const gpmpc_pack* p, int H, int K, const LbfgsLayout& L, gpmpc_solver_rule rule) {
    LbfgsWorkspace W;
    const size_t n = (size_t)H * p->da, d = sizeof(double);
    gpmpc_carver c;
    c.take(d * (size_t)L.total);
    W.off_x0 = c.take(d * K * p->ds);
    W.off_cost = c.take(d * K);
    W.off_grad = c.take(d * K * n);
    W.roll = gpmpc_solver_eval_bytes(rule, p, K, H, false, GPMPC_WANT_GRAD);
    W.off_roll = c.take(W.roll.total);
    W.total = c.total();
    return W;
}

static size_t lbfgs_solve_bytes(gpmpc_solver_rule rule, const gpmpc_pack* p, int H, const gpmpc_lbfgs_params* P) {
    if (!p || !P || P->n_starts < 1 || P->n_starts > GPMPC_LBFGS_MAX_STARTS || P->history < 1 || P->history > GPMPC_LBFGS_MAX_HISTORY) return 0;
    if (!gpmpc_solver_dims_ok(H, p->ds, p->da)) return 0;
    return lbfgs_workspace(p, H, P->n_starts, lbfgs_layout(P->n_starts, (long)H * p->da, P->history), rule).total;
}
extern "C" size_t gpmpc_lbfgs_solve_workspace_bytes(const gpmpc_pack* p, int H, const gpmpc_lbfgs_params* P) {
    return lbfgs_solve_bytes(GPMPC_RULE_DIAGONAL, p, H, P);
}
extern "C" size_t gpmpc_lbfgs_solve_fullcov_workspace_bytes(const gpmpc_pack* p, int H, const gpmpc_lbfgs_params* P) {
    return lbfgs_solve_bytes(GPMPC_RULE_FULLCOV, p, H, P);
}

// the search of both entries; the rule decides the one evaluation (solver_frame.h)
static int lbfgs_solve(gpmpc_solver_rule rule, const char* who, const gpmpc_pack* p, int H, const double* x0, const double* X0,
                       const gpmpc_cost_params* cost, const gpmpc_lbfgs_params* P, int first_tick, int n_ticks, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (!p || !x0 || !cost || !P || !workspace || H < 1 || (first_tick == 0 && !X0)) return GPMPC_E_ARG;
    if (int rc = lbfgs_check_scalars(P, who)) return rc;                 // (before the pack is looked at)
    if (first_tick < 0) return gpmpc_refuse(who, "first_tick is negative");
    if (n_ticks < 0) return gpmpc_refuse(who, "n_ticks is negative");
    if (int rc = gpmpc_solver_enter(p, H, cost, nullptr, who, [&](int da) { return gpmpc_check_bounds(P->lb, P->ub, da, who); }, rule)) return rc;
    const int K = P->n_starts, n = H * p->da;
    const LbfgsLayout L = lbfgs_layout(K, n, P->history);
    const LbfgsWorkspace W = lbfgs_workspace(p, H, K, L, rule);
    if (workspace_bytes < W.total) return GPMPC_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    double *st = (double*)ws, *x0b = (double*)(ws + W.off_x0), *cst = (double*)(ws + W.off_cost), *grd = (double*)(ws + W.off_grad);
    double* U = st + L.U;
    auto evaluate = [&]() {
        return gpmpc_solver_eval(rule, p, K, H, x0b, U, cost, nullptr, GPMPC_WANT_GRAD, cst, grd, nullptr, nullptr, ws + W.off_roll, W.roll, stream);
    };
    if (first_tick == 0) {
        if (int rc = lbfgs_launch_start(n, p->ds, p->da, *P, L, X0, nullptr, nullptr, x0, x0b, st, s)) return rc;
        if (int rc = evaluate()) return rc;
        if (int rc = lbfgs_launch_start(n, p->ds, p->da, *P, L, X0, cst, grd, nullptr, nullptr, st, s)) return rc;
    }
    for (int t = 0; t < n_ticks; ++t) {
        if (int rc = evaluate()) return rc;
        if (int rc = lbfgs_launch_tick(n, p->da, *P, L, cst, grd, st, s)) return rc;
    }
    return lbfgs_launch_finish(n, *P, L, st, s);
}

extern "C" int gpmpc_lbfgs_solve(const gpmpc_pack* p, int H, const double* x0, const double* X0, const gpmpc_cost_params* cost,
                                 const gpmpc_lbfgs_params* P, int first_tick, int n_ticks, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    return lbfgs_solve(GPMPC_RULE_DIAGONAL, "gpmpc_lbfgs_solve", p, H, x0, X0, cost, P, first_tick, n_ticks, workspace, workspace_bytes, stream);
}

extern "C" int gpmpc_lbfgs_solve_fullcov(const gpmpc_pack* p, int H, const double* x0, const double* X0, const gpmpc_cost_params* cost,
                                         const gpmpc_lbfgs_params* P, int first_tick, int n_ticks, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    return lbfgs_solve(GPMPC_RULE_FULLCOV, "gpmpc_lbfgs_solve_fullcov", p, H, x0, X0, cost, P, first_tick, n_ticks, workspace, workspace_bytes,
                       stream);
}
