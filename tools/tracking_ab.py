#!/usr/bin/env python3
"""What a cost schedule costs: ms per call of objective + gradient on ONE device, every call followed by a
synchronisation (the latency a solver loop sees), best of --blocks blocks of --reps calls, the variants interleaved within a block --

  (off)    schedule_id = 0: the plain tail kernel;
  (on)     a schedule with H + 1 different rows, input references and a terminal weight: the schedule variant of the tail;
  (on+set) the same with gpmpc_cost_schedule_set before every call -- what a closed loop that slides its window pays per step;
  (xref)   callback shapes only: tracking EMULATED with a new x_ref in the cost struct on every call, which captures the callback graph anew.

The comparison of this build with schedule_id = 0 against the parent commit's build is tools/lib_ab.py's (two builds, one process each).
Run on the GPU box:
    python tools/tracking_ab.py [N:ds:da:H:B[:cb] ...]          (":cb" = the host-in / host-out solver callback instead of gpmpc_rollout)"""
import argparse, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_process_mpc_amd as g
from gaussian_process_mpc_amd._lib import lib
from gaussian_process_mpc_amd.rollout import CostParams, CostSchedule, GPPack, rollout
from gaussian_process_mpc_amd.synth import synth_problem

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("shapes", nargs="*")
args = ap.parse_args()
shapes = args.shapes or ["512:3:1:20:1:cb", "512:3:1:20:1", "2048:4:1:20:256", "300:4:1:10:256"]
dev = g.require_gpu()

pack, last = None, None
for shape in shapes:
    f = shape.split(":")
    N, ds, da, H, B = (int(v) for v in f[:5])
    cb = len(f) > 5 and f[5] == "cb"
    if (N, ds, da) != last:
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
        last = (N, ds, da)
    rng = np.random.default_rng(5)
    Xr, Ur, Qf = rng.uniform(-1, 1, (H + 1, ds)), rng.uniform(-1, 1, (H, da)), 2.0 * pb["Q"] + 0.01
    cs = CostSchedule(H, ds, da).set(Xr, Ur, Qf)
    costs = {"off": CostParams(-1.0, pb["Q"], pb["R"]), "on": CostParams(-1.0, pb["Q"], pb["R"], schedule=cs)}
    x0, U = torch.as_tensor(pb["x0"][:B], device=dev), torch.as_tensor(pb["U"][:B, :H], device=dev)
    x0h, Uh = pb["x0"][0].copy(), pb["U"][0, :H].copy()
    step = [0]

    def run(k):
        cost = costs["off" if k == "off" else "on"]
        if k == "on+set":
            step[0] += 1
            cs.set(np.roll(Xr, step[0], axis=0), Ur, Qf)
        if k == "xref":
            step[0] += 1
            cost = CostParams(-1.0, pb["Q"], pb["R"], x_ref=Xr[step[0] % (H + 1)])
        if cb:
            return pack.objective_gradient(x0h, Uh, cost)
        r = rollout(pack, x0, U, cost, want_traj=False, graph=True)
        torch.cuda.synchronize()
        return r

    names = ["off", "on", "on+set"]
    cap0 = lib().gpmpc_pack_callback_captures(pack.handle) if cb else lib().gpmpc_pack_graph_captures(pack.handle)
    best = {k: 1e9 for k in names}
    for k in names:
        for _ in range(3):
            run(k)
    cap1 = lib().gpmpc_pack_callback_captures(pack.handle) if cb else lib().gpmpc_pack_graph_captures(pack.handle)
    for _ in range(args.blocks):
        for k in names:
            run(k)                          # untimed: the callback cache holds ONE graph, a change of cost struct captures anew
            t0 = time.perf_counter()
            for _ in range(args.reps):
                run(k)
            best[k] = min(best[k], (time.perf_counter() - t0) / args.reps)
    if cb:                                  # on its own, after the others: every call of it drops the graph the others replay
        names.append("xref")
        best["xref"] = 1e9
        for _ in range(args.blocks):
            t0 = time.perf_counter()
            for _ in range(args.reps):
                run("xref")
            best["xref"] = min(best["xref"], (time.perf_counter() - t0) / args.reps)
    form = pack.plan(B, H, graph=not cb)
    print(f"N={N} ds={ds} da={da} H={H} B={B}{' callback' if cb else ' graph'} [{form['form']} {form['tiling']}]: " +
          "  ".join(f"({k}) {best[k] * 1e3:7.3f} ms" for k in names) +
          f"   on/off x{best['on'] / best['off']:.3f}  on+set/off x{best['on+set'] / best['off']:.3f}"
          + (f"  xref/off x{best['xref'] / best['off']:.3f}" if cb else "") + f"   captures during warm-up: {cap1 - cap0}", flush=True)
    cs.close()
