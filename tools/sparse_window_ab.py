#!/usr/bin/env python3
"""What the sparse-GP window (gpmpc_sparse_remove / _replace, SparseGPState.rebase, SparseDynamics(window=...))
costs, on ONE device, in one process.  Every candidate is warmed up; a timing is a host clock around --reps calls that end in one
synchronise (the calls do not synchronise by themselves: this is the cost in a stream, as a closed loop sees it); the figure is the
MEDIAN over --blocks blocks, the candidates interleaved within a block; min and max are printed beside it.

  1. append | remove | replace | remove followed by append | rebase (accumulate over the window + inverse + finish), M in {128, 256,
     1024}, window in {400, 2000} (the window matters to the rebase only), D = 5, 2 targets.  A replace also runs against the bytes it
     must move: G, Binv and Q read and written once, 6 x 8 M^2, over the 8 TB/s of HBM (MI355X figures; at these sizes the matrices sit
     in the 256 MiB last-level cache, so this is a floor, not a prediction).
  2. closed loop: data update + pack refill per step of SparseDynamics(window=N) with the window full (every step replaces; the
     rebase every N steps is inside the mean), next to the same loop without a window (profiles/sparse/ab.txt section 3: 0.20 ms).
  3. drift: the chain of tests/test_gpu_sparse_window.py (M 33, window 48, 300 replacements, sigma_n 1e-2 and 0.1) on the device,
     max-abs difference to a fresh fit of the rows held, against the replacements since the last rebase (rebase every 48 | never).

Run on the GPU box:   python tools/sparse_window_ab.py [--out profiles/sparse/window_ab.txt] [--quick]"""
import argparse, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_process_mpc_amd as g
from gaussian_process_mpc_amd.synth import synth_problem

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=9)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--quick", action="store_true", help="small sizes only (a smoke run of the tool)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = g.require_gpu()
HBM = 8.0e12
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def medians(fns, reps):
    """{name: (median, min, max) seconds per call}: reps calls and one synchronise per timing, candidates interleaved within a block."""
    for f in fns.values():
        for _ in range(3):
            f()
        torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(args.blocks):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) / reps)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in ts.items()}


def problem(N, M, D=5, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (N, D))
    Y = np.stack((np.sin(X).sum(axis=1), np.cos(X).sum(axis=1)), axis=1) + 0.05 * rng.standard_normal((N, 2))
    lam = rng.uniform(1.0, 3.0, D)
    Z = g.select_inducing(rng.uniform(-2, 2, (max(N, M), D)), M, lam, method="random", seed=1)
    return torch.as_tensor(X, device=dev), torch.as_tensor(Y, device=dev), Z, lam


say("# sparse-GP window: tools/sparse_window_ab.py on one MI355X, median [min ... max] over %d blocks of %d calls + one synchronise" % (args.blocks, args.reps))
say("# 1. rank-one steps and the rebase, ms per call (D = 5, 2 targets; remove = (append, remove) - append, replace = (replace, replace back) / 2, remove then append = (remove, append, replace back) - replace: the state stays put)")
for M in ((128,) if args.quick else (128, 256, 1024)):
    for N in ((400,) if args.quick else (400, 2000)):
        X, Y, Z, lam = problem(N + 1, M)
        st = g.SparseGPState(Z, lam, 1.0, 0.05).fit(X[:N], Y[:N])
        st.refresh_every = 0
        xo, yo, xn, yn = X[N // 2].contiguous(), Y[N // 2].contiguous(), X[N].contiguous(), Y[N].contiguous()

        def two_calls():
            st.remove(xo, yo); st.append(xn, yn)

        def back():                                     # (undoes two_calls / replace so that the state does not wander)
            st.replace(xn, yn, xo, yo)
        # append+remove pairs keep the state where it is; each pair is timed as one call of each kind, so the single figures are halves
        snap = {k: getattr(st, k).clone() for k in ("G", "r", "Binv", "Q", "alpha", "stats")}
        b = medians({"append": lambda: st.append(xn, yn)}, args.reps)      # (the state wanders: restored below; the time does not depend on it)
        for k, t in snap.items():
            getattr(st, k).copy_(t)
        b.update(medians({"append+remove": lambda: (st.append(xn, yn), st.remove(xn, yn)),
                     "replace+replace": lambda: (st.replace(xo, yo, xn, yn), back()),
                     "remove,append+replace": lambda: (two_calls(), back())}, args.reps))
        rb = medians({"rebase": lambda: st.rebase(X[:N], Y[:N])}, max(1, args.reps // 10))["rebase"]
        rep = b["replace+replace"][0] / 2
        two = b["remove,append+replace"][0] - rep
        floor = 6.0 * 8.0 * M * M / HBM
        say("M %4d window %4d: append %7.4f [%7.4f ... %7.4f]   remove %7.4f   replace %7.4f [%7.4f ... %7.4f]   remove then append %7.4f   "
            "(replace / two calls x%.2f; 48 M^2 bytes at 8 TB/s: %.4f)   rebase %7.3f [%7.3f ... %7.3f]" %
            (M, N, b["append"][0] * 1e3, b["append"][1] * 1e3, b["append"][2] * 1e3, (b["append+remove"][0] - b["append"][0]) * 1e3, rep * 1e3,
             b["replace+replace"][1] / 2 * 1e3, b["replace+replace"][2] / 2 * 1e3, two * 1e3, rep / two, floor * 1e3,
             rb[0] * 1e3, rb[1] * 1e3, rb[2] * 1e3))
        del st
        torch.cuda.empty_cache()

say("# 2. closed loop, data update + pack refill per step (ds 2, da 1, M 32 | 128; median over the steps after 10 warm-up steps, synchronised per step)")


def loop_ms(dyn, pb, n0, steps):
    for gp in dyn.gpr_err:
        gp.set_lambdas(pb["lambdas"][0]); gp.set_sigma_n(np.array(0.05))
    dyn.append_train_data(pb["X"][:n0, :2], pb["X"][:n0, 2:], pb["Y"][:n0])
    dyn.pack()
    ts = []
    for i in range(n0, n0 + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dyn.append_train_data(pb["X"][i, :2], pb["X"][i, 2:], pb["Y"][i])
        dyn.pack()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts[10:]) * 1e3
    return float(np.median(ts)), float(np.mean(ts)), float(ts.max())


for N in ((100,) if args.quick else (400, 2000)):
    steps = N + 60                                       # one rebase (every N replacements) falls inside the timed steps
    pb = synth_problem(7, N + steps, 2, 1, 5, 2)
    for M in (32, 128):
        Z = g.select_inducing(pb["X"][:N], M, pb["lambdas"][0])
        w = loop_ms(g.SparseDynamics(2, 1, Z, window=N), pb, N, steps)
        u = loop_ms(g.SparseDynamics(2, 1, Z), pb, N, steps)
        say("N %4d M %3d: window (replace, rebase every %d) median %6.3f mean %6.3f max %6.3f ms   no window (append) median %6.3f mean %6.3f max %6.3f ms"
            % ((N, M, N) + w + u))

say("# 3. drift of a chain of replacements (M 33, window 48, D 3, 2 targets): max |state - fresh fit of the rows held| of Binv | Q | alpha | G")
rng = np.random.default_rng(4242)
n, w, M = 348, 48, 33
Xh = rng.uniform(-2, 2, (n, 3))
lamh = rng.uniform(0.7, 2.5, 3)
Zh = Xh[rng.choice(n, size=M, replace=False)] + 1e-3 * rng.standard_normal((M, 3))
for sigma_n in (1e-2, 0.1):
    Yh = np.stack([np.sin(Xh * (a + 1)).sum(axis=1) for a in range(2)], axis=1) + sigma_n * rng.standard_normal((n, 2))
    X, Y = torch.as_tensor(Xh, device=dev), torch.as_tensor(Yh, device=dev)
    for rebase_every in (48, 0):
        st = g.SparseGPState(Zh, lamh, 1.2, sigma_n).fit(X[:w], Y[:w])
        fresh = g.SparseGPState(Zh, lamh, 1.2, sigma_n)
        since, rows = 0, []
        for i in range(w, n):
            st.replace(X[i - w], Y[i - w], X[i], Y[i])
            since += 1
            if rebase_every and since >= rebase_every:
                st.rebase(X[i - w + 1:i + 1], Y[i - w + 1:i + 1])
                since = 0
            if (i - w + 1) % 12 == 0:
                fresh.fit(X[i - w + 1:i + 1], Y[i - w + 1:i + 1])
                rows.append((i - w + 1, since) + tuple(float((getattr(st, k) - getattr(fresh, k)).abs().max()) for k in ("Binv", "Q", "alpha", "G")))
        say("sigma_n %.0e, rebase every %s (max |G| %.1e): replacements (since the rebase) Binv | Q | alpha | G" %
            (sigma_n, rebase_every or "never", float(st.G.abs().max())))
        for r in rows:
            say("   %3d (%3d)  %.1e | %.1e | %.1e | %.1e" % r)

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
