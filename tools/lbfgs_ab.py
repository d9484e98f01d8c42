#!/usr/bin/env python3
"""What the device L-BFGS search costs and what it finds, on ONE device, in the protocol of tools/mppi_ab.py:

  (1) synth_problem(3, 300, 4, 1, 20, .), inputs within +-1, zero start, K in {1, 4, 16, 64}: ms per solve (a synchronisation after each
      solve, 3 fresh solves per block, best of --blocks blocks) and the cost of the returned plans for the single start (the stand-in
      gradient solver), n_starts = K on the host (the lock-step search as RiskSensitiveMPC runs it, and with the rule of the device search:
      line_points = 1, no patience) and solver="lbfgs" with check_every in {0, 8};
  (2) the pendulum closed loop of examples/pendulum_closed_loop.py (200 pre-training transitions, H = 10, 25 steps) under the same solvers
      at K = 16;
  (3) by stream events: 50 ticks of gpmpc_lbfgs_solve against 50 calls of gpmpc_rollout (B = K, with gradient) on the problem of (1) --
      their difference is what the tick kernel (and one summary kernel per call) adds per tick.

Every plan's cost is evaluated by ONE common call -- rollout(..., want_grad=False) at B = 1 -- whatever the solver reported.
Run on the GPU box:
    python tools/lbfgs_ab.py [--blocks 5] [--out profiles/lbfgs/ab.txt]"""
import argparse, ctypes, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_process_mpc_amd as g
from gaussian_process_mpc_amd._lib import lib, check, ptr, stream_ptr
from gaussian_process_mpc_amd.device_lbfgs import lbfgs_params
from gaussian_process_mpc_amd.rollout import rollout
from gaussian_process_mpc_amd.synth import synth_problem

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--steps", type=int, default=25)
ap.add_argument("--out", default=None, help="also append the table to this file")
args = ap.parse_args()
dev = g.require_gpu()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def solvers(K):
    rows = [("single start", dict())] if K == 1 else []
    if K > 1:
        rows += [(f"host n_starts={K}", dict(n_starts=K)), (f"host n_starts={K}, same rule", dict(n_starts=K, same_rule=True))]
    return rows + [(f"lbfgs x{K} check_every=0", dict(n_starts=K, solver="lbfgs", check_every=0)),
                   (f"lbfgs x{K} check_every=8", dict(n_starts=K, solver="lbfgs", check_every=8))]


def configure(mpc, cfg, seed):
    mpc.multistart_options["seed"] = seed
    if cfg.get("same_rule"):
        mpc.multistart_options.update(line_points=1, patience=None)
    if "check_every" in cfg:
        mpc.multistart_options["check_every"] = cfg["check_every"]


def plan_cost(mpc, plan):
    r = rollout(mpc.dynamics.pack(), mpc.curr_state, np.asarray(plan)[None], mpc._cost_params(), want_grad=False, want_traj=False)
    return float(r["cost"][0].item())


def solve(mpc, x, cfg, fn=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plan = (fn or mpc.get_optimal_trajectory)(x, n_starts=cfg.get("n_starts"), solver=cfg.get("solver"))
    torch.cuda.synchronize()
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


say(f"(1) synth_problem(3, 300, 4, 1, 20, .), zero start, inputs within +-1: 3 fresh solves per block, best of {args.blocks} blocks")
for K in (1, 4, 16, 64):
    for name, cfg in solvers(K):
        blocks, costs, ticks = [], [], []
        for blk in range(args.blocks + 1):                   # (the first block of every configuration is its warm-up)
            ms = []
            for rep in range(3):
                mpc = synth_mpc()
                configure(mpc, cfg, 3 * blk + rep)
                plan, t = solve(mpc, pb["x0"][0], cfg)
                ms.append(t)
                if blk:
                    costs.append(plan_cost(mpc, plan))
                    info = mpc.last_solve_info or {}
                    ticks.append(info.get("ticks", -1))
            if blk:
                blocks.append(np.mean(ms))
        say(f"    {name:32s} {min(blocks):9.2f} ms per solve (median block {np.median(blocks):9.2f})   plan cost min {min(costs):.6f} median "
            f"{np.median(costs):.6f} max {max(costs):.6f}   ticks median {int(np.median(ticks))}   [{mpc.solver_used}]")

# ---- (2) the pendulum closed loop ----------------------------------------------------------------------------------------------
say(f"(2) pendulum closed loop: 200 pre-training transitions, H = 10, {args.steps} steps, gamma = 1e-5, |u| <= 2")
for name, cfg in [("single start", dict())] + solvers(16):
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
    configure(mpc, cfg, 0)
    ms, costs, inner = [], [], mpc.get_optimal_trajectory

    def timed(obs, **kw):
        plan, t = solve(mpc, obs, cfg, inner)
        ms.append(t); costs.append(plan_cost(mpc, plan))
        return plan
    mpc.get_optimal_trajectory = timed
    hist = g.Simulator(mpc, plant, num_iters=args.steps, incremental=True).run()
    th = np.array([h[0][0] for h in hist])
    say(f"    {name:32s} {np.median(ms[1:]):9.2f} ms per solve (median; first {ms[0]:.1f})   mean plan cost {np.mean(costs):.6f}   "
        f"theta {th[0]:+.3f} -> {th[-1]:+.3f}, max |theta| {np.abs(th).max():.3f}   [{mpc.solver_used}]")

# ---- (3) the tick kernel, by stream events ---------------------------------------------------------------------------------------
say("(3) per tick, by stream events: 50 ticks of gpmpc_lbfgs_solve against 50 calls of gpmpc_rollout with gradient (problem of (1); gtol = ftol = "
    "min_step = 0: no start finishes)")
mpc = synth_mpc()
pack, cost = mpc.dynamics.pack(), mpc._cost_params()
n = H * da
for K in (1, 4, 16, 64):
    P = lbfgs_params(K, da, -1.0, 1.0, history=8, gtol=0.0, ftol=0.0, min_step=0.0)
    X0 = torch.as_tensor(np.random.default_rng(K).uniform(-1, 1, (K, n)), device=dev)
    X0[0] = 0.0
    x0 = torch.as_tensor(pb["x0"][0], device=dev)
    nbytes = lib().gpmpc_lbfgs_solve_workspace_bytes(pack.handle, H, ctypes.byref(P))
    ws = torch.zeros(nbytes // 8 + 32, dtype=torch.float64, device=dev)
    rws = pack.workspace(lib().gpmpc_rollout_workspace_bytes(pack.handle, K, H, 1))
    xb, U, cst, grd = x0.repeat(K, 1).contiguous(), X0.clone(), torch.zeros(K, dtype=torch.float64, device=dev), torch.zeros_like(X0)
    st = stream_ptr()
    state = {"first": 0}

    def run_solve(ticks):
        check(lib().gpmpc_lbfgs_solve(pack.handle, H, ptr(x0), ptr(X0), ctypes.byref(cost.c), ctypes.byref(P), state["first"], ticks,
                                      ptr(ws), ws.numel() * 8, st), "gpmpc_lbfgs_solve")
        state["first"] += ticks

    def run_rollouts(count):
        for _ in range(count):
            check(lib().gpmpc_rollout(pack.handle, K, H, ptr(xb), ptr(U), ctypes.byref(cost.c), 1, None, None, ptr(cst), ptr(grd),
                                      ctypes.c_void_p(rws.data_ptr()), rws.numel(), st), "gpmpc_rollout")
    out = {}
    for name, fn in (("solve", run_solve), ("rollout", run_rollouts), ("solve", run_solve), ("rollout", run_rollouts)):     # (second round: warm)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if name == "solve" and state["first"] == 0:
            fn(2)
        torch.cuda.synchronize()
        a.record()
        fn(50)
        b.record()
        torch.cuda.synchronize()
        out[name] = a.elapsed_time(b) / 50 * 1e3
    left = int(ws[0].item())
    say(f"    K={K:3d}: solve per tick {out['solve']:9.1f} us   gpmpc_rollout (B = K, gradient) {out['rollout']:9.1f} us   tick kernel (difference) "
        f"{out['solve'] - out['rollout']:7.1f} us = {(out['solve'] - out['rollout']) / out['rollout'] * 100:5.1f} % of the rollout   "
        f"[{pack.plan(K, H, want_grad=True)['form']}; not done {left} of {K}]")
if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
