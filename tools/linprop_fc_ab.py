#!/usr/bin/env python3
"""Timings of the full-covariance linearised rollout with state feedback on one MI355X against the DIAGONAL linearised rollout of the same
build on the same data (the existing tests pin that code to its earlier bits, so it is the reference of the ratios).

    python tools/linprop_fc_ab.py --out profiles/linprop/fc_ab.txt [--quick]

Sizes: N = 2048, ds = 4, da = 1, H = 20 for B in {1, 16, 256, 4096}; N = 300 at B = 256; a sparse model of M = 256 at B = 256.  Each size
runs objective only and with gradient, under the TILE and under the STREAM form of the step.  Method (the project's measuring guide, as
tools/linprop_ab.py): a warm-up call of both, then ``--blocks`` timed blocks in which the two rollouts ALTERNATE (``--reps`` calls of the
one, a synchronisation, ``--reps`` calls of the other, a synchronisation); reported are the median block and the spread (min ... max) in
ms per call and the ratio of the medians.  No ratio is fixed in advance.  The full rollout runs with a gain (one [da][ds] matrix): with
K = NULL it launches the same kernels."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_process_mpc_amd as G                                       # noqa: E402
from linprop_ab import fmt, models, sparse_models                          # noqa: E402


def ab_blocks(fa, fb, reps, blocks):
    """Alternating blocks of the two calls: (median, min, max) ms per call of each."""
    fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(blocks):
        for f, out in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0) / reps)
    stat = lambda t: (float(np.median(t)), float(min(t)), float(max(t)))  # noqa: E731
    return stat(ta), stat(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=5)
    a = ap.parse_args()
    G.require_gpu()
    H, ds, da = 20, 4, 1
    lines = ["# tools/linprop_fc_ab.py on %s: ms per call, median block (min ... max) of %d alternating blocks of %d calls after a warm-up; "
             "H = %d, ds = %d, da = %d; full = linearised_rollout(full_covariance=True, feedback=K), diagonal = linearised_rollout of the same build"
             % (torch.cuda.get_device_name(0), a.blocks, a.reps, H, ds, da)]

    def save():                                          # after every line: a run that is cut short leaves what it measured
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    shapes = [("N=2048 ds=4 per-GP Kinv", 2048, False, (1, 16, 256, 4096)), ("N=300 ds=4 per-GP Kinv", 300, False, (256,)),
              ("M=256 ds=4 SparseDynamics (FITC, 2048 observations)", 256, None, (256,))]
    if a.quick:
        shapes = [("N=300 ds=4 per-GP Kinv", 300, False, (16,))]
    cost = G.CostParams(-1.0, np.eye(ds), 0.1 * np.eye(da))
    rng = np.random.default_rng(1)
    K = torch.as_tensor(rng.uniform(-0.5, 0.5, (da, ds)), device="cuda")
    for name, n, shared, batches in shapes:
        keep = None
        if shared is None:
            gm, pack, keep = sparse_models(n, ds, da)
        else:
            gm, pack = models(n, ds, da, shared)
        for B in batches:
            x0 = torch.as_tensor(rng.uniform(-1, 1, (B, ds)), device="cuda")
            U = torch.as_tensor(rng.uniform(-1, 1, (B, H, da)), device="cuda")
            reps = max(1, a.reps if B <= 256 else 1)
            for form in ("tile", "stream"):
                txt = "%-52s B %5d %-6s" % (name, B, form)
                for grad, label in ((False, "objective"), (True, "with gradient")):
                    t_full, t_diag = ab_blocks(
                        lambda: G.linearised_rollout(gm, x0, U, cost, want_grad=grad, want_traj=False, form=form, full_covariance=True, feedback=K),
                        lambda: G.linearised_rollout(gm, x0, U, cost, want_grad=grad, want_traj=False, form=form), reps, a.blocks)
                    txt += " | %s: full %s diagonal %s full/diagonal %.3f" % (label, fmt(t_full), fmt(t_diag), t_full[0] / t_diag[0])
                lines.append(txt)
                print(txt, flush=True)
                save()
        del gm, pack, keep
        torch.cuda.empty_cache()
    lines.append("# not measured: the shared-Kinv shape, other ds / da / H, per-step gains, B between the listed ones, per-kernel times and hardware "
                 "counters of the new kernels, multi-GPU")
    save()


if __name__ == "__main__":
    main()
