// What csrc/lbfgs.hip shares with the solvers built on its state machine (csrc/auglag.hip): the layout of the state buffer, the check of
// the parameter scalars and the three launches.  The kernels themselves stay in lbfgs.hip; the checks every solver makes (dimensions,
// bounds, the order of a solve entry's preamble) are in solver_frame.h.
#pragma once
#include "solver_frame.h"

// offsets in doubles (include/gpmpc.h)
struct LbfgsLayout { long sum, plan, F, conv, alive, iters, ticks, done, A, cnt, head, rho, X, G, D, U, S, Y, total; };

// sections of 32 doubles = 256 bytes: the carver of gpmpc_internal.h, counted in doubles
struct lbfgs_carver {
    gpmpc_carver c;
    long take(long doubles) { return (long)(c.take(sizeof(double) * (size_t)doubles) / sizeof(double)); }
    long total() const { return (long)(c.total() / sizeof(double)); }
};
static inline LbfgsLayout lbfgs_layout(int K, long n, int m) {
    LbfgsLayout L;
    lbfgs_carver c;
    L.sum = c.take(32);
    L.plan = c.take(n);
    L.F = c.take(K); L.conv = c.take(K); L.alive = c.take(K); L.iters = c.take(K); L.ticks = c.take(K);
    L.done = c.take(K); L.A = c.take(K); L.cnt = c.take(K); L.head = c.take(K);
    L.rho = c.take((long)K * m);
    L.X = c.take(K * n); L.G = c.take(K * n); L.D = c.take(K * n); L.U = c.take(K * n);
    L.S = c.take(K * n * m); L.Y = c.take(K * n * m);
    L.total = c.total();
    return L;
}

// GPMPC_OK, or GPMPC_E_ARG with "<who>: <what>" in gpmpc_last_error
int lbfgs_check_scalars(const gpmpc_lbfgs_params* P, const char* who);          // the part of the parameters that needs no dimension

// k_lbfgs_start (cost == NULL: phase 0), k_lbfgs_tick, k_lbfgs_finish on stream s
int lbfgs_launch_start(int n, int ds, int da, const gpmpc_lbfgs_params& P, const LbfgsLayout& L, const double* X0, const double* cost,
                       const double* grad, const double* x0, double* x0b, double* st, hipStream_t s);
int lbfgs_launch_tick(int n, int da, const gpmpc_lbfgs_params& P, const LbfgsLayout& L, const double* cost, const double* grad, double* st,
                      hipStream_t s);
int lbfgs_launch_finish(int n, const gpmpc_lbfgs_params& P, const LbfgsLayout& L, double* st, hipStream_t s);
