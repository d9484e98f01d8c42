#!/usr/bin/env python3
"""What the constrained multi-start costs and what it finds, on ONE device, in the protocol of tools/mppi_ab.py:

  (1) c1 = synth_problem(1, 100, 2, 2, 10, .), gamma = 1e-5, inputs within +-1, one 95 % row on state 0 at b = top - 0.3 span of
      mu_t0 + kappa sd_t0 along the unconstrained optimum (the f = 0.3 row of tests/test_gpu_constraints.py);
  (2) synth_problem(3, 300, 4, 1, 20, .), gamma = -1, inputs within +-1, a 95 % box on state 0: one side a quarter of the way
      from a plan known to meet it (half the unconstrained plan, or 0, or its negative) to the unconstrained plan, the other side inactive;
  rows: the single start (the stand-in SLSQP, or Ipopt), solver="mppi" at K = 256, solver="auglag" at K = 1 / 4 / 16 / 64 with
  check_outer = 0 (one enqueue) and 1 (one read of the not-settled counter per outer iteration).  Per row: 5 blocks of 3 fresh solves
  (no warm start, seeds 0..2), a device synchronisation after each solve, the best block's ms per solve; every plan is priced by ONE common
  call -- rollout(..., constraints=) at B = 1 -- whatever the solver reported;
  (3) by stream events at B = K on both problems: 50 x gpmpc_rollout_constrained with gradient alone against 50 x (the same, k_al_merit,
      the tick of gpmpc_lbfgs_tick): the difference is what the solve adds to its evaluations.

Run on the GPU box:
    python tools/auglag_ab.py [--blocks 5] [--out profiles/auglag/ab.txt]"""
import argparse, ctypes, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_process_mpc_amd as g
from gaussian_process_mpc_amd._lib import WANT_GRAD, check, lib, ptr, stream_ptr
from gaussian_process_mpc_amd.device_lbfgs import lbfgs_params, lbfgs_start
from gaussian_process_mpc_amd.rollout import rollout
from gaussian_process_mpc_amd.synth import synth_problem

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--out", default=None, help="also append the table to this file")
ap.add_argument("--skip-single", action="store_true", help="leave out the single-start row (the slowest)")
args = ap.parse_args()
dev = g.require_gpu()
lines = []
K95 = 1.6448536269514722
ROWS = [("single start", dict())] * (not args.skip_single) + [("mppi K=256", dict(solver="mppi"))]
ROWS += [(f"auglag K={K} check_outer={c}", dict(solver="auglag", n_starts=K, check_outer=c)) for K in (1, 4, 16, 64) for c in (0, 1)]


def say(s):
    print(s, flush=True)
    lines.append(s)


def make_mpc(pb, gamma):
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    mpc = g.RiskSensitiveMPC(gamma, H, ds, da, pb["Q"], pb["R"])
    for a, gp in enumerate(mpc.dynamics.gpr_err):
        gp.set_lambdas(pb["lambdas"][a]); gp.set_sigma_n(float(pb["sigma_n"][a])); gp.set_sigma_f(1.0)
    mpc.dynamics.append_train_data(pb["X"][:, :ds], pb["X"][:, ds:], pb["Y"])
    mpc.set_lb([-1.0] * da); mpc.set_ub([1.0] * da)
    mpc.mppi_options.update(samples=256)
    return mpc


def priced(mpc, plan):
    r = rollout(mpc.dynamics.pack(), mpc.curr_state, np.asarray(plan)[None], mpc._cost_params(), want_grad=False, want_traj=False,
                constraints=mpc.state_constraints)
    return float(r["cost"][0].item()), float(r["g"].max().item())


def table(title, pb, gamma, box=False):
    x0 = pb["x0"][0]
    mpc = make_mpc(pb, gamma)
    U_free = mpc.get_optimal_trajectory(x0)
    e0 = np.eye(pb["ds"])[:1]

    def along(U, sign):                                      # sign mu_t0 + kappa sd_t0, t = 1..H
        r = rollout(mpc.dynamics.pack(), x0, np.asarray(U)[None], mpc._cost_params(), want_grad=False, want_traj=False,
                    constraints=g.StateConstraints(sign * e0, [0.0], kappa=K95))
        return r["g"].cpu().numpy().reshape(-1)
    if not box:
        a = along(U_free, 1.0)
        mpc.set_state_constraints(e0, [a.max() - 0.3 * (a.max() - a.min())], prob=0.95)
    else:
        # a bound that some plan is known to meet with slack (the early steps hardly depend on the inputs, so a fraction of the span along
        # the unconstrained plan need not be reachable): the first (side, plan) of which the unconstrained plan exceeds the worst value by
        # more than 5 % of its own span; the bound sits a quarter of the way from that plan to the unconstrained one
        for sign, scale in ((1.0, 0.5), (-1.0, 0.5), (1.0, 0.0), (-1.0, 0.0), (1.0, -1.0), (-1.0, -1.0)):
            a, alt = along(U_free, sign), along(scale * np.asarray(U_free), sign)
            if a.max() - alt.max() > 0.05 * (a.max() - a.min()):
                break
        else:
            raise SystemExit("no plan among 0.5 U, 0, -U gives a bound on state 0 that the unconstrained plan violates")
        bound = alt.max() + 0.25 * (a.max() - alt.max())
        far = along(U_free, -sign).max() + 1.0 + (a.max() - a.min())
        say(f"{title}: {'upper' if sign > 0 else 'lower'} bound {sign * bound:+.6f} on state 0, met with slack {bound - alt.max():.4f} by "
            f"{scale:g} x the unconstrained plan; the other side of the box lies 1 + one span beyond every value along that plan (inactive)")
        mpc.set_state_constraints(np.concatenate((sign * e0, -sign * e0)), [bound, far], prob=0.95)
    c_free, g_free = priced(mpc, U_free)
    say(f"{title}: unconstrained plan cost {c_free:.6f}, violates the bound by {g_free:.4f}; best of {args.blocks} blocks of 3 fresh solves")
    for name, cfg in ROWS:
        ms, costs, viol, extra = [], [], [], ""
        for block in range(args.blocks + 1):                 # (the first block of every row is its warm-up)
            t_block = 0.0
            for seed in range(3):
                mpc.solver_used, mpc._solve_count = None, 0
                mpc.mppi_options["seed"] = mpc.multistart_options["seed"] = seed
                if "check_outer" in cfg:
                    mpc.auglag_options["check_outer"] = cfg["check_outer"]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                plan = mpc.get_optimal_trajectory(x0, n_starts=cfg.get("n_starts"), solver=cfg.get("solver"))
                torch.cuda.synchronize()
                t_block += (time.perf_counter() - t0) * 1e3
                if block == args.blocks:
                    c, v = priced(mpc, plan)
                    costs.append(c); viol.append(v)
                    if cfg.get("solver") == "auglag":
                        extra = f"   outer {mpc.last_solve_info['outer']}, evaluations {mpc.last_solve_info['evaluations']}"
            if block:
                ms.append(t_block / 3)
        say(f"    {name:28s} {min(ms):9.2f} ms per solve (median block {np.median(ms):9.2f})   plan cost by seed "
            + " ".join(f"{c:.6f}" for c in costs) + "   max g " + " ".join(f"{v:+.1e}" for v in viol) + f"{extra}   [{mpc.solver_used}]")
    return mpc


def events(title, mpc, pb):
    pack, cost, sc = mpc.dynamics.pack(), mpc._cost_params(), mpc.state_constraints
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    n, R = H * da, H * sc.m
    e = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)  # noqa: E731
    say(f"(3) {title}: per evaluation, by stream events around 50 back-to-back calls")
    for K in (1, 4, 16, 64):
        U = torch.as_tensor(np.random.default_rng(K).uniform(-0.5, 0.5, (K, H, da)), device=dev)
        xb = torch.as_tensor(np.tile(pb["x0"][0], (K, 1)), device=dev)
        cst, grd, gv, gj, lam, rho, M, dM = e(K), e(K, n), e(K, R), e(K, R, n), e(K, R) + 0.5, e(K) + 10.0, e(K), e(K, n)
        nb = lib().gpmpc_rollout_constrained_workspace_bytes(pack.handle, K, H, WANT_GRAD)
        ws = torch.empty(nb // 8 + 32, dtype=torch.float64, device=dev)
        wsp, st = ctypes.c_void_p(ws.data_ptr()), stream_ptr()
        P = lbfgs_params(K, da, -1.0, 1.0, gtol=0.0, ftol=0.0, min_step=0.0)
        ev = lambda: lib().gpmpc_rollout_constrained(pack.handle, K, H, ptr(xb), ptr(U), ctypes.byref(cost.c), ctypes.byref(sc.c), WANT_GRAD,   # noqa: E731
                                                     None, None, ptr(cst), ptr(grd), ptr(gv), ptr(gj), wsp, ws.numel() * 8, st)
        me = lambda: lib().gpmpc_auglag_merit(K, H, da, sc.m, ptr(cst), ptr(grd), ptr(gv), ptr(gj), ptr(lam), ptr(rho), ptr(M), ptr(dM), st)   # noqa: E731
        check(ev(), "rollout"); check(me(), "merit")
        state = lbfgs_start(U, M, dM, lb=-1.0, ub=1.0, gtol=0.0, ftol=0.0, min_step=0.0)
        tk = lambda: lib().gpmpc_lbfgs_tick(H, da, ctypes.byref(P), ptr(M), ptr(dM), ptr(state), state.numel() * 8, st)   # noqa: E731

        def whole():
            rc = ev() or me()
            return rc or tk()
        out = {}
        for name, fn in (("rollout", ev), ("whole", whole), ("rollout", ev), ("whole", whole)):       # (second round: warm)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            check(fn(), name)
            torch.cuda.synchronize()
            a.record()
            for _ in range(50):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name] = a.elapsed_time(b) / 50
        say(f"    K={K:3d}: gpmpc_rollout_constrained {out['rollout'] * 1e3:9.1f} us   + k_al_merit + tick {out['whole'] * 1e3:9.1f} us   "
            f"added {(out['whole'] - out['rollout']) * 1e3:7.1f} us = {(out['whole'] - out['rollout']) / out['rollout']:.3f} of the rollout")


pb1 = synth_problem(1, 100, 2, 2, 10, 4)
m1 = table("(1) c1, the f = 0.3 row", pb1, 1e-5)
pb2 = synth_problem(3, 300, 4, 1, 20, 4)
m2 = table("(2) synth_problem(3, 300, 4, 1, 20, .), a box on state 0", pb2, -1.0, box=True)
events("c1", m1, pb1)
events("synth_problem(3, 300, 4, 1, 20, .)", m2, pb2)
if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
