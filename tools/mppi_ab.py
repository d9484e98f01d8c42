#!/usr/bin/env python3
"""What the MPPI planner costs and what it finds, on ONE device:

  (1) synth_problem(3, 300, 4, 1, 20, .), inputs within +-1, zero start: ms per solve and the cost of the returned plan for the single
      start (the stand-in gradient solver), n_starts = 16 (lock-step multi-start) and solver="mppi" at K = 64 / 256 / 1024;
  (2) the pendulum closed loop of examples/pendulum_closed_loop.py (200 pre-training transitions, H = 10, 25 steps) under the same five
      solvers: ms per solve, mean cost of the plans, where the loop ends;
  (3) by stream events: the two new kernels against the rollout between them, per iteration, at K = 64 / 256 / 1024 on the problem of (1).

Every plan's cost is evaluated by ONE common call -- rollout(..., want_grad=False) at B = 1 -- whatever the solver reported.
Run on the GPU box:
    python tools/mppi_ab.py [--reps 5] [--out profiles/mppi/ab.txt]"""
import argparse, ctypes, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_process_mpc_amd as g
from gaussian_process_mpc_amd._lib import lib, check, ptr, stream_ptr
from gaussian_process_mpc_amd.mppi import mppi_params
from gaussian_process_mpc_amd.rollout import rollout
from gaussian_process_mpc_amd.synth import synth_problem

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=25)
ap.add_argument("--out", default=None, help="also append the table to this file")
args = ap.parse_args()
dev = g.require_gpu()
lines = []
SOLVERS = [("single start", dict()), ("n_starts=16", dict(n_starts=16)), ("mppi K=64", dict(solver="mppi", K=64)),
           ("mppi K=256", dict(solver="mppi", K=256)), ("mppi K=1024", dict(solver="mppi", K=1024))]


def say(s):
    print(s, flush=True)
    lines.append(s)


def plan_cost(mpc, plan):
    r = rollout(mpc.dynamics.pack(), mpc.curr_state, np.asarray(plan)[None], mpc._cost_params(), want_grad=False, want_traj=False)
    return float(r["cost"][0].item())


def solve(mpc, x, cfg, fn=None):
    if "K" in cfg:
        mpc.mppi_options.update(samples=cfg["K"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plan = (fn or mpc.get_optimal_trajectory)(x, n_starts=cfg.get("n_starts"), solver=cfg.get("solver"))
    return plan, (time.perf_counter() - t0) * 1e3


# ---- (1) one solve on the synthetic problem -----------------------------------------------------------------------------------
pb = synth_problem(3, 300, 4, 1, 20, 4)
ds, da, H = pb["ds"], pb["da"], pb["H"]


def synth_mpc():
    mpc = g.RiskSensitiveMPC(-1.0, H, ds, da, pb["Q"], pb["R"])
    for a, gp in enumerate(mpc.dynamics.gpr_err):
        gp.set_lambdas(pb["lambdas"][a]); gp.set_sigma_n(float(pb["sigma_n"][a])); gp.set_sigma_f(1.0)
    mpc.dynamics.append_train_data(pb["X"][:, :ds], pb["X"][:, ds:], pb["Y"])
    mpc.set_lb([-1.0] * da); mpc.set_ub([1.0] * da)
    return mpc


say(f"(1) synth_problem(3, 300, 4, 1, 20, .), zero start, inputs within +-1, best of {args.reps} fresh solves")
for name, cfg in SOLVERS:
    ms, costs = [], []
    for rep in range(args.reps + 1):                         # (the first solve of every configuration is its warm-up)
        mpc = synth_mpc()
        mpc.mppi_options["seed"] = rep
        mpc.multistart_options["seed"] = rep
        plan, t = solve(mpc, pb["x0"][0], cfg)
        if rep:
            ms.append(t); costs.append(plan_cost(mpc, plan))
    say(f"    {name:14s} {min(ms):9.2f} ms per solve (median {np.median(ms):9.2f})   plan cost min {min(costs):.6f} median {np.median(costs):.6f} "
        f"max {max(costs):.6f}   [{mpc.solver_used}]")

# ---- (2) the pendulum closed loop ----------------------------------------------------------------------------------------------
say(f"(2) pendulum closed loop: 200 pre-training transitions, H = 10, {args.steps} steps, gamma = 1e-5, |u| <= 2")
for name, cfg in SOLVERS:
    rng = np.random.default_rng(0)
    plant = g.PendulumPlant()
    mpc = g.RiskSensitiveMPC(1e-5, 10, 2, 1, Q=2 * np.eye(2), R=0.001 * np.eye(1))
    for gp in mpc.dynamics.gpr_err:
        gp.set_lambdas(np.array([0.5, 0.5, 0.5])); gp.set_sigma_n(1e-3)
    S = np.column_stack((rng.uniform(-np.pi, np.pi, 200), rng.uniform(-8, 8, 200)))
    A = rng.uniform(-2, 2, (200, 1))
    NS = np.empty_like(S)
    for i in range(200):
        plant.state = S[i].copy()
        NS[i] = plant.step(A[i])[0]
    mpc.dynamics.append_train_data(S, A, NS)
    mpc.set_lb([-2.0]); mpc.set_ub([2.0]); mpc.set_xref(np.zeros(2))
    ms, costs, inner = [], [], mpc.get_optimal_trajectory

    def timed(obs, **kw):
        plan, t = solve(mpc, obs, cfg, inner)
        ms.append(t); costs.append(plan_cost(mpc, plan))
        return plan
    mpc.get_optimal_trajectory = timed
    hist = g.Simulator(mpc, plant, num_iters=args.steps, incremental=True).run()
    th = np.array([h[0][0] for h in hist])
    say(f"    {name:14s} {np.median(ms[1:]):9.2f} ms per solve (median; first {ms[0]:.1f})   mean plan cost {np.mean(costs):.6f}   "
        f"theta {th[0]:+.3f} -> {th[-1]:+.3f}, max |theta| {np.abs(th).max():.3f}   [{mpc.solver_used}]")

# ---- (3) the kernels, by stream events -----------------------------------------------------------------------------------------
say("(3) per iteration, by stream events around 50 back-to-back calls of each C entry (problem of (1))")
mpc = synth_mpc()
pack, cost = mpc.dynamics.pack(), mpc._cost_params()
n = H * da
e = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)  # noqa: E731
for K in (64, 256, 1024):
    P = mppi_params(K, da, 0.5, -1.0, 1.0, iterations=1, decay=0.9, beta=0.1, seed=1)
    mean, x0, U, xb, cst, best, best2, tr = e(n), torch.as_tensor(pb["x0"][0], device=dev), e(K, n), e(K, ds), e(K), e(2 + n), e(2 + n), e(6)
    best[:2] = float("inf")
    ws = pack.workspace(lib().gpmpc_rollout_workspace_bytes(pack.handle, K, H, 0))
    wsp, st = ctypes.c_void_p(ws.data_ptr()), stream_ptr()
    calls = {
        "sample": lambda: lib().gpmpc_mppi_sample(H, ds, da, ctypes.byref(P), 0, ptr(mean), ptr(x0), ptr(U), ptr(xb), st),
        "rollout": lambda: lib().gpmpc_rollout(pack.handle, K, H, ptr(xb), ptr(U), ctypes.byref(cost.c), 0, None, None, ptr(cst), None, wsp, ws.numel(), st),
        "update": lambda: lib().gpmpc_mppi_update(K, H, da, 0, 0.1, ptr(U), ptr(cst), None, ptr(mean), ptr(best), ptr(best2), ptr(tr), st),
    }
    out = {}
    for name in ("sample", "rollout", "update", "sample", "rollout", "update"):       # (second round: warm)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        check(calls[name](), name)
        torch.cuda.synchronize()
        a.record()
        for _ in range(50):
            calls[name]()
        b.record()
        torch.cuda.synchronize()
        out[name] = a.elapsed_time(b) / 50
    say(f"    K={K:5d}: k_mppi_sample {out['sample'] * 1e3:8.1f} us   gpmpc_rollout {out['rollout'] * 1e3:9.1f} us   k_mppi_update {out['update'] * 1e3:8.1f} us   "
        f"new kernels / rollout = {(out['sample'] + out['update']) / out['rollout']:.3f}   [{pack.plan(K, H, want_grad=False)['form']}]")
if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
