#!/usr/bin/env python3
"""Fixed-size training window: what one replacement costs and what it does to the closed loop's step time.  One GPU.

  A. device time per call of gpmpc_gp_replace and of gpmpc_gp_append at N = 256 ... 2048, D = 3 and 5, same process, same leading
     dimension of the buffers: HIP events around a batch of calls, the two alternated, several repeats; median and range.
  B. the pendulum loop of examples/pendulum_closed_loop.py, 300 steps from 200 points, refresh = "newton", with and without a window
     of 200: wall-clock per step (solve + plant + data update, ended by a device synchronise), median and p95 over steps 1-100 and
     201-300, split into the solve and the data update, with the solver callbacks per step (the windowed loop forgets the
     pre-training points, so its solves are not the unbounded loop's), how often the device pack was re-created and how often
     the callback graph was captured.

    python tools/window_probe.py [--out profiles/window/window_probe.txt] [--steps 300] [--repeats 7] [--skip-loop]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_process_mpc_amd as g                                            # noqa: E402
from gaussian_process_mpc_amd._lib import check, host_doubles, lib, stream_ptr   # noqa: E402

LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def per_call(n, D, repeats, batch):
    dev = g.require_gpu()
    rng = np.random.default_rng(n + D)
    cap = ((n + 1 + 64 + 255) // 256) * 256                 # the leading dimension GaussianProcessRegression would use
    X = torch.tensor(rng.uniform(-2, 2, (n + 1, D)), device=dev)
    lam, sf, noise = np.full(D, 1.5), 1.2, 1e-2
    d2 = ((X[:n, None, :] - X[None, :n, :]) ** 2 / torch.tensor(lam, device=dev)).sum(-1)
    src = [torch.zeros((cap, cap), dtype=torch.float64, device=dev) for _ in range(3)]
    src[0][:n, :n] = sf ** 2 * torch.exp(-0.5 * d2)
    src[1][:n, :n] = src[0][:n, :n] + noise * torch.eye(n, dtype=torch.float64, device=dev)
    src[2][:n, :n] = torch.linalg.inv(src[1][:n, :n])
    dst = [torch.zeros((cap, cap), dtype=torch.float64, device=dev) for _ in range(3)]
    nb = max(lib().gpmpc_gp_append_workspace_bytes(n, D), lib().gpmpc_gp_replace_workspace_bytes(n, D))
    ws = torch.empty(int(nb), dtype=torch.uint8, device=dev)
    _, lp = host_doubles(lam)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    X_old, xn = X[:n].contiguous(), X[n:n + 1].contiguous()
    sp = stream_ptr()

    def append():
        check(lib().gpmpc_gp_append(n, D, vp(X_old), vp(xn), lp, sf, noise, vp(src[0]), vp(src[1]), cap, vp(src[2]), cap,
                                    vp(dst[0]), vp(dst[1]), vp(dst[2]), cap, vp(ws), ws.numel(), sp), "gpmpc_gp_append")

    def replace():
        check(lib().gpmpc_gp_replace(n, D, n // 3, vp(X_old), vp(xn), lp, sf, noise, vp(src[0]), vp(src[1]), cap, vp(src[2]), cap,
                                     vp(dst[0]), vp(dst[1]), vp(dst[2]), cap, vp(ws), ws.numel(), sp), "gpmpc_gp_replace")

    times = {"append": [], "replace": []}
    for fn in (append, replace):                             # warm-up: code objects, clocks
        for _ in range(batch):
            fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for name, fn in (("append", append), ("replace", replace)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(batch):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / batch)       # microseconds per call
    med = {k: float(np.median(v)) for k, v in times.items()}
    say(f"N {n:5d} D {D}  ld {cap:5d}   append {med['append']:8.1f} us [{min(times['append']):.1f} .. {max(times['append']):.1f}]   "
        f"replace {med['replace']:8.1f} us [{min(times['replace']):.1f} .. {max(times['replace']):.1f}]   "
        f"replace / append {med['replace'] / med['append']:.3f}")
    return med


def pendulum_loop(steps, window, pretrain=200, horizon=10, incremental=True):
    rng = np.random.default_rng(0)
    plant = g.PendulumPlant()
    mpc = g.RiskSensitiveMPC(1e-5, horizon, 2, 1, Q=2 * np.eye(2), R=0.001 * np.eye(1))
    for gp in mpc.dynamics.gpr_err:
        gp.set_lambdas(np.array([0.5, 0.5, 0.5]))
        gp.set_sigma_n(1e-3)
    S = np.column_stack((rng.uniform(-np.pi, np.pi, pretrain), rng.uniform(-8, 8, pretrain)))
    A = rng.uniform(-2, 2, (pretrain, 1))
    NS = np.empty_like(S)
    for i in range(pretrain):
        plant.state = S[i].copy()
        NS[i] = plant.step(A[i])[0]
    mpc.dynamics.append_train_data(S, A, NS)
    mpc.set_lb([-2.0]); mpc.set_ub([2.0])
    mpc.set_xref(np.zeros(2))
    mpc.dynamics.max_train = window
    obs, _ = plant.reset()
    g0 = mpc.dynamics.gpr_err[0]
    ms, solve, data, evals, packs, last_pack, polishes, rebuilds = [], [], [], [], 0, None, 0, 0
    for _ in range(steps):                                   # the body of Simulator.run, timed per step
        torch.cuda.synchronize()
        CALLS[0] = 0
        t0 = time.perf_counter()
        action = mpc.get_optimal_trajectory(obs)[0, :]       # synchronous: every callback ends in a device-to-host copy
        nxt, _, _, _, _ = plant.step(action)
        t1 = time.perf_counter()
        mpc.dynamics.append_train_data(obs, action, nxt, incremental=incremental, refresh="newton" if incremental else None)
        pk = mpc.dynamics.pack()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ms.append((t2 - t0) * 1e3); solve.append((t1 - t0) * 1e3); data.append((t2 - t1) * 1e3); evals.append(CALLS[0])
        if g0._appends_since_rebuild == 0:                   # a refresh fell on this step: polish, or its fall-back to a rebuild
            if getattr(g0, "newton_steps_last", 0) == -1:
                rebuilds += 1
            else:
                polishes += 1
        packs += int(pk is not last_pack)
        last_pack = pk
        obs = nxt
    return {"ms": np.array(ms), "solve": np.array(solve), "data": np.array(data), "evals": np.array(evals), "packs": packs,
            "n_end": g0.num_train, "captures": int(lib().gpmpc_pack_callback_captures(last_pack.handle)), "polishes": polishes,
            "rebuilds": rebuilds}


CALLS = [0]
_objective_gradient = g.GPPack.objective_gradient


def _counted(self, *a, **k):
    CALLS[0] += 1
    return _objective_gradient(self, *a, **k)


g.GPPack.objective_gradient = _counted                       # solver callbacks per environment step (the solver is not this library's)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "window", "window_probe.txt"))
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--skip-loop", action="store_true")
    args = ap.parse_args()
    say(f"# tools/window_probe.py on {torch.cuda.get_device_name(0)}; {lib().gpmpc_version().decode()}")
    say(f"# A. device time per call (HIP events around {args.batch} calls, {args.repeats} repeats alternating the two; median [min .. max])")
    for D in (3, 5):
        for n in (256, 512, 1024, 2048):
            per_call(n, D, args.repeats, args.batch)
    if not args.skip_loop:
        say()
        say(f"# B. pendulum loop, {args.steps} steps from 200 points, refresh = newton; wall-clock ms per step (solve + plant + data update + pack)")
        pendulum_loop(40, None)                               # warm-up of the process (runtime, code objects, solver imports)
        for rep in range(2):
            for window in (None, 200):
                r = pendulum_loop(args.steps, window)
                for name, sl in (("steps 1-100", slice(0, 100)), (f"steps {args.steps - 99}-{args.steps}", slice(args.steps - 100, args.steps))):
                    say(f"run {rep}  window {str(window):>4s}  {name:14s}: step median {np.median(r['ms'][sl]):6.2f} p95 {np.percentile(r['ms'][sl], 95):6.2f}   "
                        f"solve median {np.median(r['solve'][sl]):6.2f}   data update + pack median {np.median(r['data'][sl]):6.3f} p95 "
                        f"{np.percentile(r['data'][sl], 95):6.3f} max {r['data'][sl].max():6.3f}   callbacks per solve median {np.median(r['evals'][sl]):5.0f}")
                say(f"run {rep}  window {str(window):>4s}  whole run     : packs created {r['packs']}  callback-graph captures of the last pack {r['captures']}  "
                    f"Newton polishes {r['polishes']}  fall-backs to a rebuild {r['rebuilds']}  final N {r['n_end']}")
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
