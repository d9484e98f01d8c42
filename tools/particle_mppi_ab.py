#!/usr/bin/env python3
"""Timings and the closed-loop effect of the particle-cost MPPI on one MI355X.

    python tools/particle_mppi_ab.py --out profiles/particles/mppi_ab.txt [--quick] [--parts abc]

Nothing here is asserted and no ratio is fixed in advance: a shape where the new rule is slower is reported like any other.  Method (the
measuring guide of the project): a warm-up call of both sides, then ALTERNATING blocks -- A, B, A, B, ... -- of ``--reps`` calls with one
synchronisation per block; reported are the median block and the spread (min ... max) of ``--blocks`` blocks per side, in ms per call.

(a) per shape -- a sparse model of M = 256, N = 300, N = 2048 with one Kinv and with a Kinv per GP; K = 64 plans, P = 256 particles, H = 20,
    ds = 4, da = 1, two constraint rows -- ms per ``particle_evaluate`` (gpmpc_particle_evaluate) against ``particle_rollout`` with its
    statistics (gpmpc_particle_rollout, which ends in gpmpc_particle_stats) at the same B P.  The rollout's kernels are unchanged code, hence
    the parent's; ``--rollout-only`` times that column alone, so that it can be run on the parent's library (GPMPC_LIB_PATH=<its build>
    GPMPC_LIB_ALLOW_MISSING=1) in the same session.  Beside it: the time of ``particle_cost`` on the
    stored particles of the same call (k_pc_step over all (plan, step) pairs in ONE launch, then k_pc_close) over the time of an evaluate,
    which launches the same workgroups step by step.  The share of the cost kernels itself comes from a kernel trace: ``--trace-shape I --calls N`` only runs N
    evaluates of shape I, for ``rocprofv3 --kernel-trace --stats -- python tools/particle_mppi_ab.py --trace-shape I``; the k_pc_* rows of its
    kernel_stats.csv over the total are the share (recorded in the profile by hand).
(b) ms per solve of ``mppi_solve_particles`` against ``mppi_solve`` (moment matching) of the same build on the same model: K = 64,
    ``--iters`` iterations, H = 20.
(c) the pendulum example with ``--max-speed``: the loop planned on particles and the loop planned by moment matching (both MPPI, same
    seeds); after every solve the plan is checked OUT OF SAMPLE, ``validate_plan(particles=4096)`` under another seed: the fraction of
    particles inside the bound per step (its minimum over the horizon) and at every step jointly."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_process_mpc_amd as G                                       # noqa: E402
from linprop_ab import fmt, models, sparse_models                          # noqa: E402  (the model builders of the sibling tool)


def alternating_ms(fa, fb, reps, blocks):
    """Median (min ... max) ms per call of fa and of fb over alternating blocks."""
    for f in (fa, fb):
        f()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(blocks):
        for k, f in enumerate((fa, fb)):
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            out[k].append(1e3 * (time.perf_counter() - t0) / reps)
    return tuple((float(np.median(o)), float(min(o)), float(max(o))) for o in out)


SHAPES = [("M=256 ds=4 SparseDynamics (FITC, 2048 observations)", 256, None), ("N=300 ds=4 per-GP Kinv", 300, False),
          ("N=2048 ds=4 shared Kinv", 2048, True), ("N=2048 ds=4 per-GP Kinv", 2048, False)]


def parts_ab(a, lines, save):
    H, ds, da, K, P = 20, 4, 1, 64, 256
    cost = G.CostParams(0.5, np.eye(ds), 0.1 * np.eye(da))
    sc = G.StateConstraints(np.array([[1.0, 0.0, 0.0, 0.0], [0.0, -1.0, 0.0, 0.0]]), [1.5, 1.5], prob=0.95)
    rng = np.random.default_rng(1)
    for name, n, shared in (SHAPES[:2] if a.quick else SHAPES):
        keep = None
        if shared is None:
            gm, pack, keep = sparse_models(n, ds, da)
        else:
            gm, pack = models(n, ds, da, shared)
        x0 = torch.as_tensor(rng.uniform(-1, 1, (K, ds)), device="cuda")
        U = torch.as_tensor(rng.uniform(-1, 1, (K, H, da)), device="cuda")
        reps = a.reps if n < 2048 else 1
        roll = lambda: G.particle_rollout(gm, x0, U, particles=P, seed=1, constraints=sc)  # noqa: E731
        if a.rollout_only:
            t = alternating_ms(roll, roll, reps, a.blocks)
            lines.append("(a) %-52s K %d P %d H %d | particle_rollout + stats of the loaded library %s | %s" % (name, K, P, H, fmt(t[0]), fmt(t[1])))
        else:
            if "a" in a.parts:
                ev = lambda: G.particle_evaluate(gm, x0, U, cost, constraints=sc, particles=P, seed=1)  # noqa: E731
                t_ev, t_roll = alternating_ms(ev, roll, reps, a.blocks)
                stored = roll()["particles"].permute(2, 0, 1, 3).contiguous()
                pc = lambda: G.particle_cost(stored, U, cost, constraints=sc)  # noqa: E731
                t_pc, _ = alternating_ms(pc, pc, a.reps, a.blocks)
                lines.append("(a) %-52s K %d P %d H %d | particle_evaluate %s | particle_rollout + stats %s | ratio %.3f | particle_cost on the stored "
                             "particles %s = %.1f %% of an evaluate" % (name, K, P, H, fmt(t_ev), fmt(t_roll), t_ev[0] / t_roll[0], fmt(t_pc),
                                                                       100.0 * t_pc[0] / t_ev[0]))
                print(lines[-1], flush=True)
                save()
                del stored
            if "b" in a.parts:
                kw = dict(samples=K, iterations=a.iters, sigma=0.5, lb=-2.0, ub=2.0, seed=1)
                xs, U0 = x0[0].cpu().numpy(), np.zeros((H, da))
                t_p, t_m = alternating_ms(lambda: G.mppi_solve_particles(gm, xs, U0, cost, constraints=sc, particles=P, **kw),
                                          lambda: G.mppi_solve(pack, xs, U0, cost, constraints=sc, **kw), 1, a.blocks)
                lines.append("(b) %-52s one MPPI solve, %d samples x %d iterations, H %d | on %d particles %s (%.1f ms per iteration) | moment matching %s | "
                             "ratio %.1f" % (name, K, a.iters, H, P, fmt(t_p), t_p[0] / a.iters, fmt(t_m), t_p[0] / t_m[0]))
        print(lines[-1], flush=True)
        save()
        del gm, pack, keep
        torch.cuda.empty_cache()


def trace_shape(a):
    """--calls evaluates of one shape of part (a) and nothing else: the program a kernel trace is taken of."""
    H, ds, da, K, P = 20, 4, 1, 64, 256
    name, n, shared = SHAPES[a.trace_shape]
    gm = sparse_models(n, ds, da)[0] if shared is None else models(n, ds, da, shared)[0]
    cost = G.CostParams(0.5, np.eye(ds), 0.1 * np.eye(da))
    sc = G.StateConstraints(np.array([[1.0, 0.0, 0.0, 0.0], [0.0, -1.0, 0.0, 0.0]]), [1.5, 1.5], prob=0.95)
    rng = np.random.default_rng(1)
    x0, U = rng.uniform(-1, 1, (K, ds)), rng.uniform(-1, 1, (K, H, da))
    for _ in range(a.calls):
        G.particle_evaluate(gm, x0, U, cost, constraints=sc, particles=P, seed=1)
    torch.cuda.synchronize()
    print("%d evaluates of %s" % (a.calls, name))


def pendulum_loop(propagation, a):
    """The loop of examples/pendulum_closed_loop.py --max-speed V --solver mppi [--propagation particles]; per step the out-of-sample check."""
    rng = np.random.default_rng(0)
    plant = G.PendulumPlant()
    mpc = G.RiskSensitiveMPC(1e-5, 10, 2, 1, Q=2 * np.eye(2), R=0.001 * np.eye(1))
    for gp in mpc.dynamics.gpr_err:
        gp.set_lambdas(np.array([0.5, 0.5, 0.5]))
        gp.set_sigma_n(1e-3)
    S = np.column_stack((rng.uniform(-np.pi, np.pi, a.pretrain), rng.uniform(-8, 8, a.pretrain)))
    A = rng.uniform(-2, 2, (a.pretrain, 1))
    NS = np.empty_like(S)
    for i in range(a.pretrain):
        plant.state = S[i].copy()
        NS[i] = plant.step(A[i])[0]
    mpc.dynamics.append_train_data(S, A, NS)
    mpc.set_lb([-2.0])
    mpc.set_ub([2.0])
    mpc.set_xref(np.zeros(2))
    mpc.propagation, mpc.solver = propagation, "mppi"
    mpc.particle_options = {"particles": 256}
    mpc.set_state_bounds([None, -a.max_speed], [None, a.max_speed], 0.95)
    solve, checks, ms = mpc.get_optimal_trajectory, [], []

    def checked(obs, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = solve(obs, **kw)
        ms.append(1e3 * (time.perf_counter() - t0))
        v = mpc.validate_plan(U=plan, x0=obs, particles=4096, seed=1000 + len(checks))
        checks.append((float(v["satisfaction"].min()), float(v["joint_satisfaction"]), bool(mpc.last_solve_info["feasible"])))
        return plan
    mpc.get_optimal_trajectory = checked
    hist = G.Simulator(mpc, plant, num_iters=a.steps, incremental=True).run()
    c = np.array([(s, j) for s, j, _ in checks])
    return dict(used=mpc.solver_used, steps=len(hist), visited=max(abs(h[0][1]) for h in hist), min_sat=c[:, 0], joint=c[:, 1],
                feasible=sum(f for _, _, f in checks), ms=float(np.median(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--rollout-only", action="store_true", help="part (a)'s rollout column alone (for a run on the parent's library)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5, help="part (b): iterations per solve")
    ap.add_argument("--pretrain", type=int, default=200)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--max-speed", type=float, default=4.0)
    ap.add_argument("--trace-shape", type=int, default=None, metavar="I", help="only run --calls evaluates of shape I of part (a), for a kernel trace")
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    G.require_gpu()
    if a.trace_shape is not None:
        trace_shape(a)
        return
    lines = ["# tools/particle_mppi_ab.py on %s: ms per call, median block (min ... max) of %d alternating blocks of %d calls (1 at N = 2048 and "
             "per solve) after a warm-up" % (torch.cuda.get_device_name(0), a.blocks, a.reps)]

    def save():                                          # after every line: a run that is cut short leaves what it measured
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    if a.rollout_only or "a" in a.parts or "b" in a.parts:
        parts_ab(a, lines, save)
    if "c" in a.parts and not a.rollout_only:
        lines.append("# (c) pendulum, |theta_dot| <= %g at 0.95 per side, H = 10, %d pre-training points, %d steps, MPPI 64 samples x 30 iterations; after "
                     "every solve validate_plan(particles=4096) under another seed" % (a.max_speed, a.pretrain, a.steps))
        for prop in ("particles", "moment_matching"):
            r = pendulum_loop(prop, a)
            lines.append("(c) planned by %-16s (%s): out-of-sample satisfaction per step, minimum over the horizon: mean %.4f, worst %.4f; jointly over the "
                         "horizon: mean %.4f, worst %.4f; solves below 0.95 per step: %d of %d; planner reports feasible in %d; largest |theta_dot| "
                         "visited %.3f; median solve %.1f ms" % (prop, r["used"], r["min_sat"].mean(), r["min_sat"].min(), r["joint"].mean(),
                                                                r["joint"].min(), int((r["min_sat"] < 0.95).sum()), r["steps"], r["feasible"],
                                                                r["visited"], r["ms"]))
            print(lines[-1], flush=True)
            save()
    lines.append("# not measured (here: the kernel trace is a run of its own, --trace-shape): hardware counters of k_pc_step / k_pc_close, P other than 256, K other than 64, other ds / da, multi-GPU")
    save()


if __name__ == "__main__":
    main()
