// The frame the device solvers share (mppi.hip, lbfgs.hip, auglag.hip): the dimension and bound checks, and the part of a solve entry's
// preamble that follows the solver's own scalar checks.  The ORDER of the checks is behaviour -- a call with two faults is refused for
// the earlier one -- and it is written down once, here.  Host only.
#pragma once
#include "gpmpc_internal.h"

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
template <class CheckInputs>
static inline int gpmpc_solver_enter(const gpmpc_pack* p, int H, const gpmpc_cost_params* cost, const gpmpc_state_constraints* cons,
                                     const char* who, CheckInputs&& check_inputs) {
    if (cons) if (int rc = gpmpc_check_constraints(cons, who)) return rc;
    if (int rc = gpmpc_check_device(p)) return rc;
    if (!gpmpc_solver_dims_ok(H, p->ds, p->da)) return GPMPC_E_ARG;
    if (int rc = check_inputs(p->da)) return rc;
    if (!p->built) return GPMPC_E_STATE;
    gpmpc_sched_ref sched;
    return gpmpc_schedule_resolve(cost, p->ds, p->da, H, who, &sched);
}
