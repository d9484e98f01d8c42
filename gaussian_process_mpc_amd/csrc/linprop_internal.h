// What the linearised rules share (linprop.hip: TILE and the dispatcher; linprop_stream.hip: STREAM; linprop_fc.hip: the full covariance):
// the model frame (model_frame.h), the tail of the model, the hyper-parameters by GP, the inputs of a step, the dispatcher's host
// interface and that of the STREAM form.  Formulas: include/gpmpc.h, "Linearised propagation".
#pragma once
#include "model_frame.h"

struct LpTail {                     // what the sums / Jacobian kernels need of the model besides the hyper-parameters
    double nom_w[GPMPC_MAX_DS * GPMPC_MAX_D], nom_b[GPMPC_MAX_DS], process_var[GPMPC_MAX_DS], action_var[GPMPC_MAX_D];
    double init_var[GPMPC_MAX_DS];  // diag(init_cov): the variance of step 0 (host side only)
    int has_nominal;
};
struct LpHyp { double ilam[GPMPC_MAX_DS][GPMPC_MAX_D]; double sf2[GPMPC_MAX_DS]; };      // 1 / lambda_ad, sf_a^2: the kernels that take GPs one by one
static inline LpHyp lp_hyp(const gpmpc_gp_model* m) {
    const int ds = m->state_dim, D = ds + m->action_dim;
    LpHyp Hy;
    memset(&Hy, 0, sizeof(Hy));
    for (int a = 0; a < ds; ++a) {
        for (int d = 0; d < D; ++d) Hy.ilam[a][d] = 1.0 / m->lambdas[a * D + d];
        Hy.sf2[a] = m->sigma_f[a] * m->sigma_f[a];
    }
    return Hy;
}
struct LpIn {                       // the inputs of a step, column c: mu + c xs, var + c xs, U + c us
    const double* mu; const double* var; const double* U;
    size_t xs, us;
};

static __device__ __forceinline__ double lp_z(const LpIn& I, int c, int d, int ds) {
    return d < ds ? I.mu[(size_t)c * I.xs + d] : I.U[(size_t)c * I.us + (d - ds)];
}

// The dispatcher of linprop.hip, also stage A of the full-covariance rule: the model checks of the diagonal entries (they fill `out`), the
// layout of one step (the form is read here, once; offsets start at 0) and the step of B columns on a workspace of gpmpc_lp_layout(...).total
// bytes -- mu_prev / var_prev: column b at + b xs; U_t: + b us; outputs at + b os; jac (or null): + b js.
struct LpLayout { size_t off_ks, off_kpart, off_part, off_hpart, off_g, total, base; int np, nbi, C, nv, form; };
int gpmpc_lp_check_model(const char* who, const gpmpc_gp_model* m, LpTail* out);
LpLayout gpmpc_lp_layout(const gpmpc_gp_model* m, int chunk, long ncols, bool want_jac);
int gpmpc_lp_step(const gpmpc_gp_model* m, const LpTail& tail, int B, const double* mu_prev, const double* var_prev, size_t xs, const double* U_t,
                  size_t us, double* out_mu, double* out_var, size_t os, double* jac, size_t js, const LpLayout& L, char* ws, hipStream_t s);

// The full-covariance rollout (linprop_fc.hip) behind gpmpc_linearised_fc_rollout and gpmpc_linearised_fc_rollout_inputs: `in` null is the
// former, launch for launch.  The launches of the commanded input's statistics (linprop_inputs.hip) are checked by their callers:
// gpmpc_lpi_cost writes out_c / out_dcovs (either may be null) and, where add_cost / add_dcovs are given, adds the same values to them.
struct LpfInputs { int input_cost; const gpmpc_input_constraints* ucons; double* out_gu; double* out_gujac; };
int gpmpc_lpf_rollout(const char* who, const gpmpc_gp_model* m, int B, int H, const double* x0, const double* U, const double* K_dev,
                      size_t k_step_stride, const gpmpc_cost_params* cost, const gpmpc_state_constraints* cons, unsigned flags, double* out_means,
                      double* out_covs, double* out_jac, double* out_cost, double* out_grad, double* out_g, double* out_gjac, int chunk,
                      void* workspace, size_t workspace_bytes, void* stream, const LpfInputs* in);
int gpmpc_lpi_check_rows(const char* who, const gpmpc_input_constraints* C);
int gpmpc_lpi_cost(int B, int H, int ds, int da, const gpmpc_cost_params* cost, const double* K, size_t k_step_stride, const double* covs,
                   double* out_c, double* out_dcovs, double* add_cost, double* add_dcovs, hipStream_t s);
int gpmpc_lpi_constraints(int B, int H, int ds, int da, const gpmpc_input_constraints* C, const double* K, size_t k_step_stride,
                          const double* U, const double* covs, const double* jac, double* out_gu, double* out_gujac, hipStream_t s);

// STREAM (linprop_stream.hip).  The bytes of a step of `ncols` columns, and the step itself on a workspace of that size (256-byte aligned);
// arguments as gpmpc_lp_step, checked by its callers.
size_t gpmpc_lps_workspace_bytes(const gpmpc_gp_model* m, long ncols, bool want_jac);
int gpmpc_lps_step(const gpmpc_gp_model* m, const LpTail& tail, int B, const double* mu_prev, const double* var_prev, size_t xs, const double* U_t,
                   size_t us, double* out_mu, double* out_var, size_t os, double* jac, size_t js, char* ws, hipStream_t s);
