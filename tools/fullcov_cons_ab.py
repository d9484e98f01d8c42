#!/usr/bin/env python3
"""What the chance constraints cost on the full-covariance rollout, on one MI355X.

    python tools/fullcov_cons_ab.py --out profiles/fullcov/cons_ab.txt [--quick]

Three calls of the same build on the same data alternate: ``rollout_fullcov(constraints=sc)`` (gpmpc_rollout_fullcov_constrained),
``rollout_fullcov`` (gpmpc_rollout_fullcov: the difference is the pack kernel and the sweep) and ``rollout(constraints=sc)``
(gpmpc_rollout_constrained, the diagonal rule: the ratio is the cost of the full rule).  Sizes: N = 2048 and N = 300, ds = 4, da = 1,
H = 20, B in {1, 16, 256}, three rows (an axis row, two general ones), objective only and with gradient.  Then one MPPI solve (64 samples, 30
iterations) and one augmented-Lagrangian solve (4 starts, 8 x 25 ticks, all outer iterations enqueued) under either rule.  Method (the
project's measuring guide, as tools/linprop_fc_ab.py): a warm-up call of each, then ``--blocks`` timed blocks in which the calls ALTERNATE
(``--reps`` calls of one, a synchronisation, the next); reported are the median block and the spread (min ... max) in ms per call and the
ratios of the medians.  No number is fixed in advance."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_process_mpc_amd as G                                       # noqa: E402
from linprop_ab import fmt, models                                         # noqa: E402


def alternate(calls, reps, blocks):
    """Alternating blocks of the calls: (median, min, max) ms per call of each."""
    for f in calls:
        f()
    torch.cuda.synchronize()
    times = [[] for _ in calls]
    for _ in range(blocks):
        for f, out in zip(calls, times):
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0) / reps)
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=5)
    a = ap.parse_args()
    G.require_gpu()
    H, ds, da = 20, 4, 1
    lines = ["# tools/fullcov_cons_ab.py on %s: ms per call, median block (min ... max) of %d alternating blocks of %d calls after a warm-up; "
             "H = %d, ds = %d, da = %d, 3 rows; fc+cons = rollout_fullcov(constraints=), fc = rollout_fullcov, diag+cons = rollout(constraints=)"
             % (torch.cuda.get_device_name(0), a.blocks, a.reps, H, ds, da)]

    def save():                                          # after every line: a run that is cut short leaves what it measured
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def say(txt):
        lines.append(txt)
        print(txt, flush=True)
        save()
    shapes = [("N=2048", 2048, (1, 16, 256)), ("N=300", 300, (1, 16, 256))]
    if a.quick:
        shapes = [("N=300", 300, (1, 16))]
    cost = G.CostParams(-1.0, np.eye(ds), 0.1 * np.eye(da))
    rng = np.random.default_rng(1)
    rows = rng.standard_normal((3, ds))
    rows[0] = 0.0
    rows[0, 0] = 1.0
    sc = G.StateConstraints(rows, np.array([0.5, 0.2, 0.1]), kappa=np.array([1.645, 2.0, 0.0]))
    for name, n, batches in shapes:
        _, pack = models(n, ds, da, False)
        pack.enable_fullcov()
        for B in batches:
            x0 = torch.as_tensor(rng.uniform(-1, 1, (B, ds)), device="cuda")
            U = torch.as_tensor(rng.uniform(-1, 1, (B, H, da)), device="cuda")
            txt = "%-7s B %4d %-28s" % (name, B, pack.plan_fullcov(B, H)["form"])
            for grad, label in ((False, "objective"), (True, "with gradient")):
                t = alternate([lambda: G.rollout_fullcov(pack, x0, U, cost, want_grad=grad, constraints=sc),
                               lambda: G.rollout_fullcov(pack, x0, U, cost, want_grad=grad),
                               lambda: G.rollout(pack, x0, U, cost, want_grad=grad, want_traj=False, constraints=sc)], a.reps, a.blocks)
                txt += (" | %s: fc+cons %s fc %s diag+cons %s  (fc+cons)/fc %.3f  (fc+cons)/(diag+cons) %.2f"
                        % (label, fmt(t[0]), fmt(t[1]), fmt(t[2]), t[0][0] / t[1][0], t[0][0] / t[2][0]))
            say(txt)
        # one solve of each device solver under either rule (wall time of the whole call, results copied out)
        x0 = rng.uniform(-1, 1, ds)
        X0 = rng.uniform(-1, 1, (4, H, da))
        mp = dict(constraints=sc, samples=64, iterations=30, sigma=0.5, lb=-1.0, ub=1.0)
        al = dict(lb=-1.0, ub=1.0, outer=8, inner_ticks=25, check_outer=0)
        t = alternate([lambda: G.mppi_solve(pack, x0, np.zeros((H, da)), cost, full_covariance=True, **mp),
                       lambda: G.mppi_solve(pack, x0, np.zeros((H, da)), cost, **mp),
                       lambda: G.auglag_solve(pack, x0, X0, cost, sc, full_covariance=True, **al),
                       lambda: G.auglag_solve(pack, x0, X0, cost, sc, **al)], 1, 3 if not a.quick else 1)
        say("%-7s solves, ms per solve: mppi 64 x 30 full %s diagonal %s ratio %.2f | auglag 4 starts 8 x 25 full %s diagonal %s ratio %.2f"
            % (name, fmt(t[0]), fmt(t[1]), t[0][0] / t[1][0], fmt(t[2]), fmt(t[3]), t[2][0] / t[3][0]))
        del pack
        torch.cuda.empty_cache()
    say("# not measured: other ds / da / H / numbers of rows, the one-lambda (shared) cross-unit form, B between and beyond the listed ones, "
        "per-kernel times and hardware counters of k_fc_pack_jac and the sweep, the L-BFGS solve, multi-GPU")


if __name__ == "__main__":
    main()
