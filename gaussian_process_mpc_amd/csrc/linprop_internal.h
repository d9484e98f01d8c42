// What the two forms of the linearised step share (linprop.hip: TILE and the dispatcher; linprop_stream.hip: STREAM): the tail of the model,
// the inputs of a step, and the host interface of the STREAM form.  Formulas: include/gpmpc.h, "Linearised propagation".
#pragma once
#include "gpmpc_internal.h"

struct LpTail {                     // what the sums / Jacobian kernels need of the model besides the hyper-parameters
    double nom_w[GPMPC_MAX_DS * GPMPC_MAX_D], nom_b[GPMPC_MAX_DS], process_var[GPMPC_MAX_DS], action_var[GPMPC_MAX_D];
    double init_var[GPMPC_MAX_DS];  // diag(init_cov): the variance of step 0 (host side only)
    int has_nominal;
};
struct LpIn {                       // the inputs of a step, column c: mu + c xs, var + c xs, U + c us
    const double* mu; const double* var; const double* U;
    size_t xs, us;
};

static __device__ __forceinline__ double lp_z(const LpIn& I, int c, int d, int ds) {
    return d < ds ? I.mu[(size_t)c * I.xs + d] : I.U[(size_t)c * I.us + (d - ds)];
}

// The dispatcher of linprop.hip for the full-covariance rule (linprop_fc.hip), whose stage A is the diagonal step itself: the model checks
// of the diagonal entries, the layout of one step (the form is read here, once; offsets start at 0) and the step on a workspace of
// gpmpc_lp_layout(...).total bytes.  Arguments as lp_step of linprop.hip.
struct LpLayout { size_t off_ks, off_kpart, off_part, off_hpart, off_g, total, base; int np, nbi, C, nv, form; };
int gpmpc_lp_check_model(const char* who, const gpmpc_gp_model* m, LpTail* out);
LpLayout gpmpc_lp_layout(const gpmpc_gp_model* m, int chunk, long ncols, bool want_jac);
int gpmpc_lp_step(const gpmpc_gp_model* m, const LpTail& tail, int B, const double* mu_prev, const double* var_prev, size_t xs, const double* U_t,
                  size_t us, double* out_mu, double* out_var, size_t os, double* jac, size_t js, const LpLayout& L, char* ws, hipStream_t s);

// STREAM (linprop_stream.hip).  The bytes of a step of `ncols` columns, and the step itself on a workspace of that size (256-byte aligned);
// arguments as lp_step of linprop.hip, checked by its callers.
size_t gpmpc_lps_workspace_bytes(const gpmpc_gp_model* m, long ncols, bool want_jac);
int gpmpc_lps_step(const gpmpc_gp_model* m, const LpTail& tail, int B, const double* mu_prev, const double* var_prev, size_t xs, const double* U_t,
                   size_t us, double* out_mu, double* out_var, size_t os, double* jac, size_t js, char* ws, hipStream_t s);
