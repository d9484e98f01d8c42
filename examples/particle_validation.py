#!/usr/bin/env python3
"""How good are the moment-matched predictions of a plan?  Pendulum, pre-trained GP, ONE solve under a chance bound on theta_dot, then
RiskSensitiveMPC.validate_plan: the same plan rolled out with particles through the GPs' pointwise posterior, next to the moments the
solver worked with.

    python examples/particle_validation.py [--pretrain 200] [--horizon 10] [--particles 4096] [--prob 0.95] [--max-speed 4.0]
                                           [--inducing M] [--seed 0]

Printed per horizon step: moment-matched and Monte-Carlo mean / standard deviation of each state, their difference in Monte-Carlo
standard errors, the empirical satisfaction of each constraint row next to the requested probability, and -- over the whole horizon --
the joint satisfaction and the mean realised stage cost.  --inducing M: the same with FITC sparse GP dynamics on M inducing points.

Needs an MI355X and the built library."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussian_process_mpc_amd import LinearNominalModel, PendulumPlant, RiskSensitiveMPC, select_inducing   # noqa: E402


def pendulum_mpc(prob=0.95, inducing=0, pretrain=200, horizon=10, max_speed=4.0, gamma=1e-5):
    """The controller of examples/pendulum_closed_loop.py --nominal identity --max-speed, pre-trained; returns (mpc, start state)."""
    rng = np.random.default_rng(0)
    plant = PendulumPlant()
    mpc = RiskSensitiveMPC(gamma, horizon, 2, 1, Q=2 * np.eye(2), R=0.001 * np.eye(1), nominal_models=LinearNominalModel.identity(2, 1))
    for gp in mpc.dynamics.gpr_err:
        gp.set_lambdas(np.array([0.5, 0.5, 0.5]))
        gp.set_sigma_n(1e-3)
    S = np.column_stack((rng.uniform(-np.pi, np.pi, pretrain), rng.uniform(-8, 8, pretrain)))
    A = rng.uniform(-2, 2, (pretrain, 1))
    NS = np.empty_like(S)
    for i in range(pretrain):
        plant.state = S[i].copy()
        NS[i] = plant.step(A[i])[0]
    if inducing:
        mpc.use_inducing_points(select_inducing(np.column_stack((S, A)), inducing, np.array([0.5, 0.5, 0.5])))
    mpc.dynamics.append_train_data(S, A, NS)
    mpc.set_lb([-2.0])
    mpc.set_ub([2.0])
    mpc.set_xref(np.zeros(2))
    if max_speed is not None:
        mpc.set_state_bounds([None, -max_speed], [None, max_speed], prob)
    return mpc, np.array([2.0, 0.0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pretrain", type=int, default=200)
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--particles", type=int, default=4096)
    ap.add_argument("--prob", type=float, default=0.95, help="one-sided satisfaction probability of the bound on |theta_dot|")
    ap.add_argument("--max-speed", type=float, default=4.0)
    ap.add_argument("--inducing", type=int, default=0, metavar="M", help="sparse GP dynamics on M inducing points (FITC)")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    mpc, x0 = pendulum_mpc(a.prob, a.inducing, a.pretrain, a.horizon, a.max_speed)
    mpc.get_optimal_trajectory(x0)
    print("one solve: %s %s" % (mpc.solver_used, mpc.last_solve_info if mpc.last_solve_info is not None else ""))
    v = mpc.validate_plan(particles=a.particles, seed=a.seed)
    names = ("theta", "theta_dot")
    print("%d particles; per step t: moment-matched | Monte-Carlo | difference in standard errors" % v["particles"])
    print("  t  " + "  ".join("%-58s" % ("%s: mean mm / mc (z)   sd mm / mc (z of var)" % n) for n in names) + "  satisfied (requested %s)"
          % np.round(v["requested"], 3).tolist())
    for t in range(a.horizon + 1):
        cells = []
        for k in range(2):
            cells.append("%+8.4f / %+8.4f (%+5.2f)   %7.4f / %7.4f (%+5.2f)    "
                         % (v["mean_mm"][t, k], v["mean_mc"][t, k], v["z_mean"][t, k], np.sqrt(max(v["var_mm"][t, k], 0.0)),
                            np.sqrt(max(v["var_mc"][t, k], 0.0)), v["z_var"][t, k]))
        sat = "" if t == 0 else "  " + " ".join("%.4f" % s for s in v["satisfaction"][t - 1])
        print(" %2d  %s%s" % (t, "  ".join(cells), sat))
    print("joint satisfaction of every row at every step: %.4f; particles with a clamped variance per step: %s; mean realised stage cost %.4f"
          % (v["joint_satisfaction"], v["clamped"].tolist(), v["stage_cost"]))


if __name__ == "__main__":
    main()
