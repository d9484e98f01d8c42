// What fullcov.hip shares with fullcov_cons.hip: the arguments of a full-covariance rollout call, which name the four step-Jacobian arrays
// both forms of the rollout leave in the workspace, and the rollout itself as an internal entry that hands them back.
#pragma once
#include "gpmpc_internal.h"

struct FcArgs {
    int B, H, ds, da, D, grad;
    const double* x0; const double* U;
    double* u; double* S;                 // [B][D], [B][D][D]   inputs of the current step
    double* mean; double* cov;            // [B][ds], [B][ds][ds] outputs of the current step
    double* out_means; double* out_covs;  // [B][H+1][ds], [B][H+1][ds][ds]
    // Jacobians of every step t = 1..H at slice t-1: [H][B][...]
    double* dmean_du; double* dmean_dS; double* dcov_du; double* dcov_dS;
    double* out_cost; double* out_grad;
    gpmpc_cost_params cost;
    const double* sched; int sched_hmax;   // cost schedule of the call (include/gpmpc.h), read by k_fc_tail<DS, true> only, else null
    const double* noise;                   // noise model of the pack (gpmpc_pack::noise_dev), read by k_fc_assemble
};

// k_fc_tail (fullcov.hip): its LU workers, the bytes of its dynamic LDS for a horizon, their ceiling, and the state dimensions it is
// instantiated for.  A call that runs the tail outside these is GPMPC_E_ARG -- in gpmpc_rollout_fullcov where it has always been, in the
// entries of fullcov_cons.hip and the *_solve_fullcov entries before their first launch (gpmpc_fc_refuse).
#define GPMPC_FC_WORKERS 32
#define GPMPC_FC_TAIL_LDS_MAX ((size_t)60 * 1024)
#define GPMPC_FC_TAIL_MAX_DS 6
static inline size_t gpmpc_fc_tail_lds(int ds_, int da, int H) {
    const size_t ds = ds_, D = ds + da, nz = ds + ds * ds;
    return sizeof(double) * ((size_t)GPMPC_FC_WORKERS * ds * 2 * ds + (H + 1) + (size_t)(H + 1) * nz + 2 * nz + D + D * D + 2 * (size_t)H * da);
}

// gpmpc_rollout_fullcov (fullcov.hip) with two additions: *out_args (or null) receives the arguments the kernels ran with -- with
// GPMPC_WANT_GRAD its four Jacobian pointers lie in `workspace` and hold every step once the stream gets there --, and tail = false ends
// the call after the last step: no cost, no reverse sweep (cost, out_cost and out_grad are then not looked at).  Every check precedes
// the first launch.  With tail = true and out_args = null this IS gpmpc_rollout_fullcov.
int gpmpc_fc_run(const gpmpc_pack* p, int B, int H, const double* x0, const double* U, const gpmpc_cost_params* cost, unsigned flags, bool tail,
                 double* out_means, double* out_covs, double* out_cost, double* out_grad, void* workspace, size_t workspace_bytes,
                 void* stream, FcArgs* out_args);
