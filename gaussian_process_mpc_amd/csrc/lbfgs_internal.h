// What csrc/lbfgs.hip shares with the solvers built on its state machine (csrc/auglag.hip): the layout of the state buffer, the checks of
// the parameters and the three launches.  The kernels themselves stay in lbfgs.hip.
#pragma once
#include "gpmpc_internal.h"

// offsets in doubles (include/gpmpc.h)
struct LbfgsLayout { long sum, plan, F, conv, alive, iters, ticks, done, A, cnt, head, rho, X, G, D, U, S, Y, total; };

static inline long lbfgs_r(long x) { return (x + 31) & ~31L; }
static inline LbfgsLayout lbfgs_layout(int K, long n, int m) {
    LbfgsLayout L;
    long o = 0;
    L.sum = o; o += 32;
    L.plan = o; o += lbfgs_r(n);
    L.F = o; o += lbfgs_r(K);
    L.conv = o; o += lbfgs_r(K);
    L.alive = o; o += lbfgs_r(K);
    L.iters = o; o += lbfgs_r(K);
    L.ticks = o; o += lbfgs_r(K);
    L.done = o; o += lbfgs_r(K);
    L.A = o; o += lbfgs_r(K);
    L.cnt = o; o += lbfgs_r(K);
    L.head = o; o += lbfgs_r(K);
    L.rho = o; o += lbfgs_r((long)K * m);
    L.X = o; o += lbfgs_r(K * n);
    L.G = o; o += lbfgs_r(K * n);
    L.D = o; o += lbfgs_r(K * n);
    L.U = o; o += lbfgs_r(K * n);
    L.S = o; o += lbfgs_r(K * n * m);
    L.Y = o; o += lbfgs_r(K * n * m);
    L.total = o;
    return L;
}

// GPMPC_OK, or GPMPC_E_ARG with "<who>: <what>" in gpmpc_last_error
int lbfgs_refuse(const char* who, const char* what);
int lbfgs_check_scalars(const gpmpc_lbfgs_params* P, const char* who);          // the part of the parameters that needs no dimension
int lbfgs_check_inputs(const gpmpc_lbfgs_params* P, int da, const char* who);   // lb <= ub of every input
int lbfgs_dims_ok(int H, int ds, int da);

// k_lbfgs_start (cost == NULL: phase 0), k_lbfgs_tick, k_lbfgs_finish on stream s
int lbfgs_launch_start(int n, int ds, int da, const gpmpc_lbfgs_params& P, const LbfgsLayout& L, const double* X0, const double* cost,
                       const double* grad, const double* x0, double* x0b, double* st, hipStream_t s);
int lbfgs_launch_tick(int n, int da, const gpmpc_lbfgs_params& P, const LbfgsLayout& L, const double* cost, const double* grad, double* st,
                      hipStream_t s);
int lbfgs_launch_finish(int n, const gpmpc_lbfgs_params& P, const LbfgsLayout& L, double* st, hipStream_t s);
