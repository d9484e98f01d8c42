#!/usr/bin/env python3
"""What the state chance constraints cost: ms per call on ONE device, three variants per shape --

  (a) gpmpc_rollout with gradient, plain launches (the unconstrained code path, unchanged);
  (b) gpmpc_rollout_constrained with gradient: the same rollout as one batch + k_rollout_constraints (values and the dense Jacobian);
  (c) k_rollout_constraints alone, through gpmpc_rollout_constraints on a trajectory and step Jacobians that are already there.

Every call is followed by a synchronisation (the latency a solver loop sees); best of --blocks blocks of --reps calls, the variants
interleaved within a block.  (b) - (a) is what a constrained callback adds; (c) is the kernel's own launch + run + wait.
Run on the GPU box:
    python tools/constraints_ab.py [N:ds:da:H:B:m_c ...] [--out profiles/constraints/ab.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/constraints_ab.py --blocks 1 300:4:1:20:256:8      (the kernel's own time)"""
import argparse, ctypes, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_process_mpc_amd as g
from gaussian_process_mpc_amd._lib import lib, check, ptr, stream_ptr
from gaussian_process_mpc_amd.rollout import CostParams, GPPack, StateConstraints, rollout, rollout_constraints
from gaussian_process_mpc_amd.synth import synth_problem

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None, help="also append the table to this file")
ap.add_argument("shapes", nargs="*")
args = ap.parse_args()
# C1 and C2 at B = 1 (BASELINE.json), and a batch: N = 300, ds = 4, H = 20, B = 256 with 2 and 8 rows
shapes = args.shapes or ["100:2:2:10:1:3", "512:3:1:20:1:3", "300:4:1:20:256:2", "300:4:1:20:256:8"]
dev = g.require_gpu()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


pack, last = None, None
for shape in shapes:
    N, ds, da, H, B, m_c = (int(v) for v in shape.split(":"))
    if (N, ds, da, H) != last:
        pack = None
        torch.cuda.empty_cache()
        pb = synth_problem(3, N, ds, da, H, max(B, 2))
        kinv = []
        for a in range(ds):
            gp = g.GaussianProcessRegression(ds + da)
            gp.set_lambdas(pb["lambdas"][a]); gp.set_sigma_f(np.array(1.0)); gp.set_sigma_n(np.array(pb["sigma_n"][a]))
            gp.append_train_data(pb["X"], pb["Y"][:, a]); kinv.append(gp.Ky_inv)
        pack = GPPack(pb["X"], pb["Y"], torch.stack(kinv), pb["lambdas"], pb["sigma_f"])
        del kinv
        last = (N, ds, da, H)
    rng = np.random.default_rng(m_c)
    sc = StateConstraints(rng.standard_normal((m_c, ds)), rng.standard_normal(m_c), kappa=rng.uniform(0.5, 2.5, m_c))
    cost = CostParams(-1.0, pb["Q"], pb["R"])
    x0, U = torch.as_tensor(pb["x0"][:B], device=dev), torch.as_tensor(pb["U"][:B, :H], device=dev)
    # inputs of (c): a trajectory and its step Jacobians
    e = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)  # noqa: E731
    means, vars_, jac = e(B, H + 1, ds), e(B, H + 1, ds), e(B, H, 2 * ds, 2 * ds + da)
    ws = pack.workspace(lib().gpmpc_rollout_jac_workspace_bytes(pack.handle, B, H))
    check(lib().gpmpc_rollout_jac(pack.handle, B, H, ptr(x0), ptr(U), ptr(means), ptr(vars_), ptr(jac), ctypes.c_void_p(ws.data_ptr()),
                                  ws.numel(), stream_ptr()), "gpmpc_rollout_jac")
    torch.cuda.synchronize()

    def run(k):
        if k == "a":
            r = rollout(pack, x0, U, cost, want_traj=False)
        elif k == "b":
            r = rollout(pack, x0, U, cost, want_traj=False, constraints=sc)
        else:
            r = rollout_constraints(means, vars_, jac, sc, ds, da)
        torch.cuda.synchronize()
        return r

    best = {k: 1e9 for k in "abc"}
    for k in best:
        for _ in range(3):
            run(k)
    for _ in range(args.blocks):
        for k in best:
            t0 = time.perf_counter()
            for _ in range(args.reps):
                run(k)
            best[k] = min(best[k], (time.perf_counter() - t0) / args.reps)
    plan = pack.plan(B, H)
    jac_mb = B * H * m_c * H * da * 8 / 1e6
    say(f"N={N} ds={ds} da={da} H={H} B={B} m_c={m_c} [{plan['form']} split={plan['split']}]: (a) rollout {best['a'] * 1e3:8.3f} ms   "
        f"(b) constrained {best['b'] * 1e3:8.3f} ms   (c) kernel alone {best['c'] * 1e3:8.3f} ms   (b)-(a) {1e3 * (best['b'] - best['a']):+8.3f} ms   "
        f"Jacobian {jac_mb:.3f} MB")
if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
