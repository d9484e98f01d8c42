#!/usr/bin/env python3
"""What the linear nominal model costs ("Linear nominal model"): ms per call of objective + gradient on ONE device, three packs
per shape --

  (a) no nominal model, default plan (one launch per step / whole horizon where the thresholds choose them);
  (b) no nominal model under GPMPC_FUSED=0 GPMPC_FUSED_SB=0 GPMPC_PERSIST=0: the two-launch form a nominal pack is planned in;
  (c) nominal model on (identity on the states, 0.05 on the actions, bias 0.01).

Every call is followed by a synchronisation (the latency a solver loop sees); best of --blocks blocks of --reps calls, the three packs
interleaved within a block.  Then, with per-launch timing on (plain launches), the pair-kernel time per launch of classes 0 (full) and
1 (horizon step 1) for (b), (c) and (b) again: (c) must sit within the spread of the two (b) runs -- no pair kernel knows the model.
Run on the GPU box:
    python tools/nominal_ab.py [N:ds:da:H:B[:cb] ...]          (":cb" = the host-in / host-out solver callback instead of gpmpc_rollout)"""
import argparse, ctypes, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_process_mpc_amd as g
from gaussian_process_mpc_amd._lib import lib
from gaussian_process_mpc_amd.rollout import CostParams, GPPack, rollout
from gaussian_process_mpc_amd.synth import synth_problem

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("shapes", nargs="*")
args = ap.parse_args()
shapes = args.shapes or ["512:3:1:20:1", "512:3:1:20:1:cb", "2048:4:1:20:256", "300:4:1:10:256"]
OVR = ("GPMPC_FUSED", "GPMPC_FUSED_SB", "GPMPC_PERSIST")
dev = g.require_gpu()


def pair_times():
    out = []
    for cls in (0, 1):
        ms, n = ctypes.c_double(), ctypes.c_longlong()
        lib().gpmpc_pair_kernel_time_class(cls, ctypes.byref(ms), ctypes.byref(n))
        out.append(ms.value / max(n.value, 1) * 1e3)
    lib().gpmpc_pair_kernel_time(None, None, 1)
    return out


packs, last = {}, None
for shape in shapes:
    f = shape.split(":")
    N, ds, da, H, B = (int(v) for v in f[:5])
    cb = len(f) > 5 and f[5] == "cb"
    if (N, ds, da) != last:
        packs.clear(); torch.cuda.empty_cache()
        pb = synth_problem(3, N, ds, da, H, max(B, 2))
        kinv = []
        for a in range(ds):
            gp = g.GaussianProcessRegression(ds + da)
            gp.set_lambdas(pb["lambdas"][a]); gp.set_sigma_f(np.array(1.0)); gp.set_sigma_n(np.array(pb["sigma_n"][a]))
            gp.append_train_data(pb["X"], pb["Y"][:, a]); kinv.append(gp.Ky_inv)
        kinv = torch.stack(kinv)
        W = np.concatenate((np.eye(ds), np.full((ds, da), 0.05)), axis=1)
        packs["a"] = GPPack(pb["X"], pb["Y"], kinv, pb["lambdas"], pb["sigma_f"])
        for k in OVR:
            os.environ[k] = "0"
        packs["b"] = GPPack(pb["X"], pb["Y"], kinv, pb["lambdas"], pb["sigma_f"])
        for k in OVR:
            os.environ.pop(k)
        packs["c"] = GPPack(pb["X"], pb["Y"], kinv, pb["lambdas"], pb["sigma_f"], nominal=(W, np.full(ds, 0.01)))
        del kinv
        last = (N, ds, da)
    cost = CostParams(-1.0, pb["Q"], pb["R"])
    x0, U = torch.as_tensor(pb["x0"][:B], device=dev), torch.as_tensor(pb["U"][:B, :H], device=dev)
    x0h, Uh = pb["x0"][0].copy(), pb["U"][0, :H].copy()

    def run(p, graph=True):
        if cb:
            return p.objective_gradient(x0h, Uh, cost)
        r = rollout(p, x0, U, cost, want_traj=False, graph=graph)
        torch.cuda.synchronize()
        return r

    best = {k: 1e9 for k in packs}
    for k in packs:
        for _ in range(3):
            run(packs[k])
    for _ in range(args.blocks):
        for k in packs:
            t0 = time.perf_counter()
            for _ in range(args.reps):
                run(packs[k])
            best[k] = min(best[k], (time.perf_counter() - t0) / args.reps)
    forms = {k: packs[k].plan(B, H, graph=True) for k in packs}
    print(f"N={N} ds={ds} da={da} H={H} B={B}{' callback' if cb else ' graph'}: " +
          "  ".join(f"({k}) {best[k] * 1e3:7.3f} ms [{forms[k]['form']} {forms[k]['tiling']} split={forms[k]['split']}]" for k in packs) +
          f"   (c)/(b) x{best['c'] / best['b']:.3f}  (c)/(a) x{best['c'] / best['a']:.3f}", flush=True)
    if not cb:
        lib().gpmpc_timing_enable(1)
        lib().gpmpc_pair_kernel_time(None, None, 1)
        rows = []
        for k in ("b", "c", "b"):
            for _ in range(args.reps):
                run(packs[k], graph=False)
            rows.append((k, pair_times()))
        lib().gpmpc_timing_enable(0)
        print("    pair kernel, us per launch [class 0 full | class 1 first step]: " +
              "   ".join(f"({k}) {t[0]:8.2f} | {t[1]:8.2f}" for k, t in rows), flush=True)
