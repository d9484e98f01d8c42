// The frame the device solvers share (mppi.hip, lbfgs.hip, auglag.hip): the dimension and bound checks, and the part of a solve entry's
// preamble that follows the solver's own scalar checks.  The ORDER of the checks is behaviour -- a call with two faults is refused for
// the earlier one -- and it is written down once, here.  Host only.
#pragma once
#include "gpmpc_internal.h"

// The rule a solve evaluates its batches with: the diagonal moment-matched rollout (the entries that have always existed) or the
// full-covariance one (the *_fullcov entries).  State machines, state layouts and the checks below are shared.
enum gpmpc_solver_rule { GPMPC_RULE_DIAGONAL = 0, GPMPC_RULE_FULLCOV = 1 };

// H, ds, da a solver can take: n = H da columns as blockIdx.y in units of 64 (as in constraints.hip)
static inline int gpmpc_solver_dims_ok(int H, int ds, int da) {
    return H >= 1 && da >= 1 && da <= GPMPC_MAX_D && ds >= 0 && ds <= GPMPC_MAX_DS && (long)H * da <= 64L * 65535;
}

// lb <= ub of every input: GPMPC_OK, or GPMPC_E_ARG with the text (lb > ub, or a NaN bound)
static inline int gpmpc_check_bounds(const double* lb, const double* ub, int da, const char* who) {
    for (int j = 0; j < da; ++j)
        if (!(lb[j] <= ub[j])) return gpmpc_refuse(who, "lb[%d] = %g exceeds ub[%d] = %g", j, lb[j], j, ub[j]);
    return GPMPC_OK;
}

// What a *_solve entry checks after its null checks and its parameter scalars (those need no pack and come first):
//   cons (if given) -> the device -> dimensions -> check_inputs(da), the solver's per-input parameters -> built -> the cost schedule
// (the rollouts of the solve would refuse a bad cost schedule too, but only after the first kernels of the solve)
// (under GPMPC_RULE_FULLCOV, after `built`: what gpmpc_rollout_fullcov refuses in a pack and of a horizon, gpmpc_fc_refuse)
template <class CheckInputs>
static inline int gpmpc_solver_enter(const gpmpc_pack* p, int H, const gpmpc_cost_params* cost, const gpmpc_state_constraints* cons,
                                     const char* who, CheckInputs&& check_inputs, gpmpc_solver_rule rule = GPMPC_RULE_DIAGONAL) {
    if (cons) if (int rc = gpmpc_check_constraints(cons, who)) return rc;
    if (int rc = gpmpc_check_device(p)) return rc;
    if (!gpmpc_solver_dims_ok(H, p->ds, p->da)) return GPMPC_E_ARG;
    if (int rc = check_inputs(p->da)) return rc;
    if (!p->built) return GPMPC_E_STATE;
    if (rule == GPMPC_RULE_FULLCOV) {
        if (int rc = gpmpc_fc_refuse(p, who, H)) return rc;
    }
    gpmpc_sched_ref sched;
    return gpmpc_schedule_resolve(cost, p->ds, p->da, H, who, &sched);
}

// The ONE evaluation site of a solve, behind the rule.  cons null: cost (and gradient); else also g (and g_jac).  flags: GPMPC_WANT_GRAD or 0.
// GPMPC_RULE_DIAGONAL makes exactly the call the solver has always made; GPMPC_RULE_FULLCOV keeps the trajectory in the head of `ws`
// (gpmpc_rollout_fullcov has no optional outputs).
struct gpmpc_solver_eval_layout { size_t off_means, off_covs, off_roll, roll_bytes, total; };
static inline gpmpc_solver_eval_layout gpmpc_solver_eval_bytes(gpmpc_solver_rule rule, const gpmpc_pack* p, int K, int H, bool cons,
                                                               unsigned flags) {
    gpmpc_solver_eval_layout L = {0, 0, 0, 0, 0};
    if (rule == GPMPC_RULE_DIAGONAL) {
        L.roll_bytes = cons ? gpmpc_rollout_constrained_workspace_bytes(p, K, H, flags) : gpmpc_rollout_workspace_bytes(p, K, H, flags);
        L.total = L.roll_bytes;
        return L;
    }
    gpmpc_carver c;
    if (!cons) {
        L.off_means = c.take(sizeof(double) * K * (H + 1) * p->ds);
        L.off_covs = c.take(sizeof(double) * K * (H + 1) * p->ds * p->ds);
    }
    L.roll_bytes = cons ? gpmpc_rollout_fullcov_constrained_workspace_bytes(p, K, H, flags) : gpmpc_rollout_fullcov_workspace_bytes(p, K, H, flags);
    L.off_roll = c.take(L.roll_bytes);
    L.total = c.total();
    return L;
}
static inline int gpmpc_solver_eval(gpmpc_solver_rule rule, const gpmpc_pack* p, int K, int H, const double* x0b, const double* U,
                                    const gpmpc_cost_params* cost, const gpmpc_state_constraints* cons, unsigned flags, double* cst,
                                    double* grd, double* g, double* gjac, char* ws, const gpmpc_solver_eval_layout& L, void* stream) {
    if (rule == GPMPC_RULE_DIAGONAL) {
        if (cons) return gpmpc_rollout_constrained(p, K, H, x0b, U, cost, cons, flags, nullptr, nullptr, cst, grd, g, gjac, ws, L.roll_bytes, stream);
        return gpmpc_rollout(p, K, H, x0b, U, cost, flags, nullptr, nullptr, cst, grd, ws, L.roll_bytes, stream);
    }
    if (cons)
        return gpmpc_rollout_fullcov_constrained(p, K, H, x0b, U, cost, cons, flags, nullptr, nullptr, cst, grd, g, gjac, ws + L.off_roll,
                                                 L.roll_bytes, stream);
    return gpmpc_rollout_fullcov(p, K, H, x0b, U, cost, flags, (double*)(ws + L.off_means), (double*)(ws + L.off_covs), cst, grd,
                                 ws + L.off_roll, L.roll_bytes, stream);
}
