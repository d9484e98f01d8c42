#!/usr/bin/env python3
"""Closed-loop risk-sensitive GP-MPC on the pendulum plant, the shape of the reference's
src/experiments/pretrain_uncertainty.py: pre-train the GP on random transitions, then run the MPC loop
(Simulator.run, src/simulator.py:37-60) with the model growing by one observation per step.

    python examples/pendulum_closed_loop.py [--pretrain 200] [--steps 25] [--horizon 10] [--window N] [--nominal identity]
                                            [--max-speed V [--prob P]] [--solver mppi [--samples K] [--iters I]] [--solver lbfgs [--starts K]]
                                            [--max-speed V --solver auglag [--starts K]] [--track AMPLITUDE,PERIOD [--terminal W]]
                                            [--obs-var V [--process-var sigma_n]] [--inducing M [--inducing-select farthest|random]]
                                            [--propagation particles --solver mppi [--particles P]]

--window N: fixed-size training window -- once the model holds N points every new observation replaces the oldest one (first-in
first-out), so the cost of the data update and the memory stay constant however long the loop runs (what the solver makes of a model
that has forgotten its pre-training points is another matter: BASELINE.md section 4w).

--nominal identity: the GPs learn the state DIFFERENCE x_{t+1} - x_t (LinearNominalModel.identity: the nominal model of state a is
x_a) and the rollout adds the state back exactly; a zero-mean GP on the raw next state reverts to 0 away from the data.

--max-speed V [--prob P]: chance bound |theta_dot| <= V on every predicted state, each side held with probability P (default 0.95) on
the predicted mean plus Phi^-1(P) predicted standard deviations (RiskSensitiveMPC.set_state_bounds).  The stand-in solver is then scipy's
SLSQP on the objective / gradient / constraints / jacobian callbacks -- one device pass per iterate.

--solver mppi [--samples K] [--iters I]: the sampling planner on the device (RiskSensitiveMPC.solver = "mppi", mppi.py): K perturbed copies
of the previous plan per iteration as one objective-only batch, no gradient; with --max-speed the bound is its feasibility rule.  Works
with --nominal identity (the rollout honours the model).

--solver lbfgs [--starts K]: the lock-step multi-start L-BFGS search with its state machine on the device (RiskSensitiveMPC.solver =
"lbfgs", device_lbfgs.py): K starts, one batched rollout with gradient and one small kernel per tick, no host in between.  Not with
--max-speed (the search is unconstrained).

--solver auglag [--starts K]: the constrained multi-start on the device (RiskSensitiveMPC.solver = "auglag", device_auglag.py): an augmented
Lagrangian over the batched constrained rollout, K starts, multipliers and penalties updated on the device.  Needs --max-speed.

--track AMPLITUDE,PERIOD [--terminal W]: theta follows AMPLITUDE cos(2 pi k / PERIOD) (k in MPC steps) instead of being regulated to 0:
the reference window of every step goes into the controller's ONE cost schedule (RiskSensitiveMPC.reference = fn), whose rows live in
device memory -- the solver-callback graph is captured once for the whole loop (printed: gpmpc_pack_callback_captures), where calling
set_xref every step would capture it every step.  --terminal W: terminal weight W Q on the last predicted state (mpc.Q_terminal).

--obs-var V [--process-var sigma_n]: the controller sees the state through Gaussian measurement noise of variance V (per component) and is
told so: V I is the covariance of the start state of every prediction (RiskSensitiveMPC.set_initial_covariance -- where an estimator runs, its
covariance goes there, before every solve; the values live in device memory, the callback graph is captured once).  --process-var sigma_n
adds each GP's noise variance to its predicted variance at every step: the spread of the next STATE, not of the latent function.

--propagation particles --solver mppi [--particles P]: the planner scores every sample on P Monte-Carlo particles through the GP posterior
(RiskSensitiveMPC.propagation = "particles", particles.mppi_solve_particles): the entropic risk of the stage cost over the particles, and with
--max-speed the empirical quantile of |theta_dot| - V in the place of mean + kappa sd.  No gradients: it needs --solver mppi.  Works with
--nominal identity, --inducing and --window.

--inducing M [--inducing-select farthest|random]: sparse GP dynamics (RiskSensitiveMPC.use_inducing_points, sparse.py): M inducing points
chosen among the pre-training inputs summarise ALL observations (FITC); every new observation is an O(M^2) rank-one update on the device
and the rollout's cost depends on M only, so neither grows with the loop (printed: the data-update time of the first and the last
quarter of the steps, and the one pack handle / callback capture of the whole loop).  With --window N the sparse model holds the newest
N observations: once full, every observation replaces the oldest one by an O(M^2) rank-one replacement (use_inducing_points(Z, window=N)).

Needs an MI355X and the built library; no gym, no cyipopt (the stand-in solver is scipy's L-BFGS-B on the same
objective / gradient callbacks, so the trajectories are NOT the reference's Ipopt trajectories)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussian_process_mpc_amd import LinearNominalModel, PendulumPlant, RiskSensitiveMPC, Simulator, select_inducing   # noqa: E402


class NoisyObservation(object):
    """The plant seen through additive Gaussian measurement noise of variance ``var`` per component (the plant's own state stays exact)."""

    def __init__(self, plant, var, rng):
        self.plant, self.sd, self.rng = plant, float(np.sqrt(var)), rng

    def _see(self, obs):
        return np.asarray(obs, dtype=np.float64) + self.sd * self.rng.standard_normal(np.shape(obs))

    def reset(self):
        obs, info = self.plant.reset()
        return self._see(obs), info

    def step(self, action):
        obs, *rest = self.plant.step(action)
        return (self._see(obs), *rest)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pretrain", type=int, default=200)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--gamma", type=float, default=1e-5)
    ap.add_argument("--starts", type=int, default=1, help="K > 1: lock-step multi-start solve, one batched rollout per tick (mpc.n_starts)")
    ap.add_argument("--window", type=int, default=None, help="fixed-size training window of N points (Simulator max_train); default: the set grows")
    ap.add_argument("--refresh", choices=("rebuild", "newton"), default=None, help="how the incremental path bounds its round-off")
    ap.add_argument("--nominal", choices=("none", "identity"), default="none", help="identity: the GPs learn x_{t+1} - x_t, the rollout adds x_t back")
    ap.add_argument("--max-speed", type=float, default=None, help="chance bound on |theta_dot| over the horizon (state constraints)")
    ap.add_argument("--prob", type=float, default=0.95, help="one-sided satisfaction probability of --max-speed")
    ap.add_argument("--solver", choices=("default", "mppi", "lbfgs", "auglag"), default="default",
                    help="mppi: the sampling planner on the device; lbfgs: the multi-start L-BFGS search on the device (--starts K); "
                         "auglag: the constrained multi-start on the device (--max-speed V, --starts K)")
    ap.add_argument("--samples", type=int, default=64, help="--solver mppi: samples per iteration")
    ap.add_argument("--iters", type=int, default=30, help="--solver mppi: iterations per solve")
    ap.add_argument("--track", default=None, metavar="AMPLITUDE,PERIOD", help="theta follows AMPLITUDE cos(2 pi k / PERIOD), k in MPC steps")
    ap.add_argument("--terminal", type=float, default=None, help="terminal weight W Q on the last predicted state (mpc.Q_terminal)")
    ap.add_argument("--obs-var", type=float, default=None, metavar="V", help="measurement-noise variance on what the controller sees; V I is its initial covariance")
    ap.add_argument("--process-var", choices=("sigma_n",), default=None, help="sigma_n: add each GP's noise variance to its predicted variance")
    ap.add_argument("--inducing", type=int, default=None, metavar="M", help="sparse GP dynamics on M inducing points (FITC), chosen among the pre-training inputs")
    ap.add_argument("--inducing-select", choices=("farthest", "random"), default="farthest", help="how --inducing picks its points")
    ap.add_argument("--propagation", choices=("moment_matching", "moment_matching_full", "linearised", "linearised_full", "particles"), default="moment_matching",
                    help="linearised: first-order propagation mu' = m(z), var' = s2(z) + grad m^T S grad m (mpc.propagation); with the default solver, --starts K or --solver mppi.  "
                         "linearised_full: the same rule with the whole covariance, predicted under --feedback.  "
                         "moment_matching_full: exact moment matching with the whole covariance (chance rows on a^T Sigma a), every solver; not with --nominal.  "
                         "particles: cost and chance rows on --particles Monte-Carlo particles; needs --solver mppi")
    ap.add_argument("--particles", type=int, default=256, metavar="P", help="with --propagation particles: particles per sample (1 ... 4096; mpc.particle_options)")
    ap.add_argument("--feedback", choices=("none", "lqr"), default="none",
                    help="with --propagation linearised_full: lqr predicts under u = v + K (x - mu) with the LQR gain of the model linearised at the upright rest "
                         "(linearised.lqr_gain with the controller's Q and R; mpc.set_feedback_gain)")
    ap.add_argument("--input-prob", type=float, default=None, metavar="P",
                    help="with --feedback lqr: chance constraints on the COMMANDED input u = v + K (x - mu): each actuator bound holds with "
                         "probability P (mpc.set_input_chance_bounds); the out-of-sample figure is validate_plan(feedback=True) on the last plan")
    ap.add_argument("--feedback-input-cost", action="store_true",
                    help="with --feedback lqr: charge tr(R K Sigma K^T), the spread of the commanded input (mpc.feedback_input_cost)")
    ap.add_argument("--linearised-form", choices=("tile", "stream", "auto"), default=None,
                    help="with --propagation linearised: the form of the linearised step (mpc.linearised_form); stream is the matrix-vector form for B = 1")
    args = ap.parse_args()
    if args.window is not None and args.window < 1:
        ap.error("--window must be >= 1")
    if args.propagation in ("linearised", "linearised_full") and args.solver in ("lbfgs", "auglag"):
        ap.error("--propagation %s runs with the default solver, --starts K or --solver mppi (the device L-BFGS / augmented Lagrangian: not yet)" % args.propagation)
    if args.propagation == "particles" and args.solver != "mppi":
        ap.error("--propagation particles needs --solver mppi (there are no gradients through particles)")
    if not 1 <= args.particles <= 4096:
        ap.error("--particles must lie in 1...4096")
    if args.feedback != "none" and args.propagation != "linearised_full":
        ap.error("--feedback needs --propagation linearised_full")
    if (args.input_prob is not None or args.feedback_input_cost) and args.feedback == "none":
        ap.error("--input-prob and --feedback-input-cost need --feedback lqr (without a gain the commanded input has no spread)")
    if args.propagation == "moment_matching_full" and args.nominal != "none":
        ap.error("--propagation moment_matching_full does not combine with --nominal (the full-covariance rollout knows no nominal model)")
    if args.propagation == "moment_matching_full" and args.max_speed is not None and args.starts > 1 and args.solver == "default":
        ap.error("--propagation moment_matching_full with --max-speed and --starts K > 1 needs --solver auglag")

    rng = np.random.default_rng(0)
    plant = PendulumPlant()
    if args.track is not None:                           # start on the reference: the first point of the sinusoid, at rest
        amp, period = (float(v) for v in args.track.split(","))
        plant = PendulumPlant(init_state=(amp, 0.0))
    nominal = LinearNominalModel.identity(2, 1) if args.nominal == "identity" else None
    mpc = RiskSensitiveMPC(args.gamma, args.horizon, 2, 1, Q=2 * np.eye(2), R=0.001 * np.eye(1), nominal_models=nominal)
    for gp in mpc.dynamics.gpr_err:                      # hypers before data, as in pretrain_uncertainty.py:100-105
        gp.set_lambdas(np.array([0.5, 0.5, 0.5]))
        gp.set_sigma_n(1e-3)
    # random transitions around the whole state space
    S = np.column_stack((rng.uniform(-np.pi, np.pi, args.pretrain), rng.uniform(-8, 8, args.pretrain)))
    A = rng.uniform(-2, 2, (args.pretrain, 1))
    NS = np.empty_like(S)
    for i in range(args.pretrain):
        plant.state = S[i].copy()
        NS[i] = plant.step(A[i])[0]
    if args.inducing is not None:
        if not 1 <= args.inducing <= args.pretrain:
            ap.error("--inducing must lie in 1...--pretrain")
        mpc.use_inducing_points(select_inducing(np.column_stack((S, A)), args.inducing, np.array([0.5, 0.5, 0.5]), method=args.inducing_select),
                                window=args.window)                # (the sparse model's own window: max_train is the dense one's)
    mpc.dynamics.append_train_data(S, A, NS)
    mpc.set_lb([-2.0]); mpc.set_ub([2.0])
    mpc.set_xref(np.zeros(2))
    mpc.n_starts = args.starts
    mpc.propagation = args.propagation
    mpc.linearised_form = args.linearised_form
    mpc.particle_options = {"particles": args.particles}
    if args.feedback == "lqr":
        from gaussian_process_mpc_amd import lqr_gain
        K = lqr_gain(mpc.dynamics, np.zeros(2), np.zeros(1), 2 * np.eye(2), 0.001 * np.eye(1))
        mpc.set_feedback_gain(K)
        print("feedback: LQR gain K = %s" % np.array2string(K, precision=4))
        mpc.feedback_input_cost = args.feedback_input_cost
        if args.input_prob is not None:
            mpc.set_input_chance_bounds(args.input_prob)
    if args.solver == "mppi":
        mpc.solver = "mppi"
        mpc.mppi_options.update(samples=args.samples, iterations=args.iters)
    if args.solver == "lbfgs":
        mpc.solver = "lbfgs"
    if args.solver == "auglag":
        if args.max_speed is None:
            ap.error("--solver auglag needs --max-speed (without constraints use --solver lbfgs)")
        mpc.solver = "auglag"
    track = None
    if args.track is not None:
        w = 2.0 * np.pi / period

        def track(k):                                    # (theta, theta_dot) of steps k .. k + H; theta_dot in rad/s (dt = plant.dt)
            t = np.arange(k, k + args.horizon + 1)
            return np.column_stack((amp * np.cos(w * t), -amp * w / plant.dt * np.sin(w * t)))
        mpc.reference = track
    if args.terminal is not None:
        mpc.Q_terminal = args.terminal * 2 * np.eye(2)
    solves = []
    if args.max_speed is not None:
        mpc.set_state_bounds([None, -args.max_speed], [None, args.max_speed], args.prob)
        solve = mpc.get_optimal_trajectory

        def logged(obs, **kw):                           # keep every step's solver report
            plan = solve(obs, **kw)
            if mpc.last_solve_info is not None:          # (None while the model is empty, or under Ipopt)
                solves.append(dict(mpc.last_solve_info))
            return plan
        mpc.get_optimal_trajectory = logged

    env = plant
    if args.obs_var is not None or args.process_var is not None:
        if args.obs_var is not None and not args.obs_var >= 0.0:
            ap.error("--obs-var must be >= 0")
        mpc.set_noise_model(process_var=args.process_var)
        if args.obs_var is not None:
            env = NoisyObservation(plant, args.obs_var, np.random.default_rng(1))
            mpc.set_initial_covariance(args.obs_var * np.eye(2))      # (constant here; an estimator would hand in its P before every solve)

    data_ms = []
    if args.inducing is not None:                        # time every data update of the loop (synchronised: the update is asynchronous)
        import torch
        feed, handle0 = mpc.dynamics.append_train_data, mpc.dynamics.pack().handle

        def timed(*a, **kw):
            torch.cuda.synchronize()
            t = time.perf_counter()
            feed(*a, **kw)
            mpc.dynamics.pack()
            torch.cuda.synchronize()
            data_ms.append((time.perf_counter() - t) * 1e3)
        mpc.dynamics.append_train_data = timed

    sim = Simulator(mpc, env, num_iters=args.steps, incremental=True, refresh=args.refresh,
                    max_train=None if args.inducing is not None else args.window)
    t0 = time.perf_counter()
    hist = sim.run()
    dt = time.perf_counter() - t0
    th = np.array([h[0][0] for h in hist])
    print(f"{len(hist)} MPC steps in {dt:.2f} s ({dt / len(hist) * 1e3:.1f} ms per step, solver: {mpc.solver_used}); "
          f"training set {args.pretrain} -> {mpc.dynamics.gpr_err[0].num_train} points"
          + (f" (window of {args.window}, next slot {mpc.dynamics.window_slot})" if args.window else "")
          + (f"; nominal model: {args.nominal}" if nominal else ""))
    if args.inducing is not None:
        from gaussian_process_mpc_amd import lib
        q = max(1, len(data_ms) // 4)
        st = mpc.dynamics._groups[0][1]
        print(f"sparse GP: {args.inducing} inducing points ({args.inducing_select}) for {mpc.dynamics.num_train} observations, min Lambda {st.min_lambda:.3e}; "
              f"data update + pack refill {np.mean(data_ms[:q]):.3f} ms per step over the first {q} steps, {np.mean(data_ms[-q:]):.3f} ms over the last {q}; "
              f"pack handle kept: {mpc.dynamics.pack().handle is handle0}, "
              f"gpmpc_pack_callback_captures = {lib().gpmpc_pack_callback_captures(mpc.dynamics.pack().handle)}")
    if args.feedback == "lqr":
        # the last plan from the last state, out of sample: particles under the gain against the actuator bounds
        from gaussian_process_mpc_amd import InputConstraints
        had = mpc.input_constraints
        if had is None:                                  # (count against the bounds also where they were not imposed)
            mpc.input_constraints = InputConstraints.box([-2.0], [2.0], 1, prob=0.95 if args.input_prob is None else args.input_prob)
        v = mpc.validate_plan(x0=hist[-1][0], particles=4096, seed=1, feedback=True)
        mpc.input_constraints = had
        print("commanded input under the gain, last plan, 4096 particles: satisfaction of |u| <= 2 per step, worst row %.4f, joint %.4f "
              "(requested %s); input sd, particles %.3g ... %.3g, linearised_full %.3g ... %.3g" % (
                  v["input_satisfaction"].min(), v["joint_input_satisfaction"], "none" if args.input_prob is None else "%.2f per bound" % args.input_prob,
                  np.sqrt(v["input_cov_mc"].min()), np.sqrt(v["input_cov_mc"].max()), np.sqrt(v["input_cov_lf"].min()), np.sqrt(v["input_cov_lf"].max())))
    if args.max_speed is not None:
        sp = np.array([abs(h[0][1]) for h in hist])
        print(f"|theta_dot| <= {args.max_speed} with probability {args.prob}: largest visited {sp.max():.3f}; "
              f"{sum(s['success'] for s in solves)} of {len(solves)} solves report success, "
              f"largest predicted violation {max((s['max_violation'] for s in solves), default=float('nan')):.2e}")
    if track is not None:
        from gaussian_process_mpc_amd import lib
        want = np.array([track(k)[0, 0] for k in range(len(th))])
        print(f"tracking {args.track}: RMS error of theta {np.sqrt(np.mean((th - want) ** 2)):.4f} rad over {len(th)} steps "
              f"(second half: {np.sqrt(np.mean((th - want)[len(th) // 2:] ** 2)):.4f}); "
              f"gpmpc_pack_callback_captures = {lib().gpmpc_pack_callback_captures(mpc.dynamics.pack().handle)}")
    if args.obs_var is not None or args.process_var is not None:
        P, av, w = mpc.dynamics.pack().noise
        print(f"noise model: init_cov diag {np.diag(P)}, action_var {av}, process_var {w}"
              + (f"; true theta at the end {plant.state[0]:.3f} (seen: {th[-1]:.3f})" if args.obs_var is not None else ""))
    print("theta:", np.array2string(th[:: max(1, len(th) // 10)], precision=2))


if __name__ == "__main__":
    main()
