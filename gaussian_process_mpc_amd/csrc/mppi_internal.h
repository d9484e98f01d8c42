// The MPPI search, written once for its three evaluations: the pack rollouts (mppi.hip), the linearised rollout (linprop.hip) and the
// particle cost (particle_cost.hip).  An entry makes its own checks in its own order, carves the head below and then its evaluation's
// workspace, and hands the search a callable that enqueues one evaluation.  Host only.
#pragma once
#include "solver_frame.h"

// mppi.hip.  The parameter checks: the part that needs no dimension (a null P: a bare GPMPC_E_ARG), then sigma and the bounds input by
// input; and the launch of k_mppi_sample on checked arguments.
int gpmpc_mppi_check_scalars(const gpmpc_mppi_params* P, const char* who);
int gpmpc_mppi_check_inputs(const gpmpc_mppi_params* P, int da, const char* who);
int gpmpc_mppi_launch_sample(int H, int ds, int da, const gpmpc_mppi_params& P, int iteration, const double* mean, const double* x0, double* U,
                             double* x0b, hipStream_t s);

// the head of a solve's workspace: U [K][n] | x0 [K][ds] | cost [K] | g [K][H m_c] | mean [n] | best x 2 [2 + n], n = H da
struct gpmpc_mppi_head { size_t off_U, off_x0, off_cost, off_g, off_mean, off_best[2]; };
static inline gpmpc_mppi_head gpmpc_mppi_head_take(gpmpc_carver& c, int H, int ds, int da, int K, int m_c) {
    gpmpc_mppi_head L;
    const size_t n = (size_t)H * da, d = sizeof(double);
    L.off_U = c.take(d * K * n);
    L.off_x0 = c.take(d * K * ds);
    L.off_cost = c.take(d * K);
    L.off_g = c.take(d * K * H * m_c);
    L.off_mean = c.take(d * n);
    L.off_best[0] = c.take(d * (2 + n));
    L.off_best[1] = c.take(d * (2 + n));
    return L;
}

// The search on checked arguments: per iteration the sample kernel, eval(it, x0b, U, cst, g) -- it enqueues the cost [K] and, with m_c > 0,
// the constraint values g [K][H m_c] of the K plans U from the start states x0b, and returns a GPMPC_* code -- and the update kernel.
template <class Eval>
static inline int gpmpc_mppi_search(const gpmpc_mppi_head& L, char* ws, int H, int ds, int da, int m_c, const gpmpc_mppi_params* P,
                                    const double* x0, const double* start, Eval&& eval, double* out_U, double* out_best, double* out_trace,
                                    void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int K = P->n_samples, n = H * da;
    double *U = (double*)(ws + L.off_U), *x0b = (double*)(ws + L.off_x0), *cst = (double*)(ws + L.off_cost);
    double* g = m_c ? (double*)(ws + L.off_g) : nullptr;
    double *mean = (double*)(ws + L.off_mean), *best[2] = {(double*)(ws + L.off_best[0]), (double*)(ws + L.off_best[1])};
    // best = (+inf, +inf, start plan), mean = start plan
    const double key0[2] = {__builtin_huge_val(), __builtin_huge_val()};
    if (int rc = gpmpc_upload_small(best[0], key0, sizeof(key0), s)) return rc;
    GPMPC_HIP(hipMemcpyAsync(best[0] + 2, start, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    GPMPC_HIP(hipMemcpyAsync(mean, start, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    for (int it = 0; it < P->iterations; ++it) {
        if (int rc = gpmpc_mppi_launch_sample(H, ds, da, *P, it, mean, x0, U, x0b, s)) return rc;
        if (int rc = eval(it, (const double*)x0b, (const double*)U, cst, g)) return rc;
        if (int rc = gpmpc_mppi_update(K, H, da, m_c, P->beta, U, cst, g, mean, best[it & 1], best[(it + 1) & 1], out_trace + 6 * (size_t)it, stream))
            return rc;
    }
    const double* fin = best[P->iterations & 1];
    GPMPC_HIP(hipMemcpyAsync(out_best, fin, sizeof(double) * 2, hipMemcpyDeviceToDevice, s));
    GPMPC_HIP(hipMemcpyAsync(out_U, fin + 2, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    return GPMPC_OK;
}
