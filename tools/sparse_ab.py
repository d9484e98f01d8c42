#!/usr/bin/env python3
"""What the sparse GP (FITC inducing points) costs and saves, on ONE device.  Protocol of tools/nominal_ab.py: every
call is followed by a synchronisation, best of --blocks blocks of --reps calls, the candidates interleaved within a block.

  1. fit: gpmpc_sparse_accumulate over N rows, D = 5, one target, default chunk, against
       (a) the same two products through torch.matmul (rocBLAS fp64) on a materialised chunk of k(Z, X_c), same chunk size;
       (b) 3 N M^2 flops (N M^2 for V = W K with the triangle of W used, 2 N M^2 for G, whose two triangles are both counted although
           only one is computed) over the 78.6 TFLOP/s fp64 vector peak DESIGN.md section 5 uses.
     Both forms of the products are timed: scalar fp64 FMA on 4 x 4 register tiles and v_mfma_f64_16x16x4_f64 (gpmpc_sparse_set_form).
  2. append (rank one) and refresh (inverse of B + finish) over M.
  3. closed loop: data update + pack refill per step, SparseDynamics (M = 32, 128) against the dense incremental path
     (Dynamics.append_train_data(incremental=True), unchanged by the sparse GP) at N = 400 and 2000.
  4. the planner's side: one solver callback (B = 1) and the C3-shape batch (ds 4, da 1, H 20, B 256) on a pack of M = 256 inducing
     points against the dense pack of N = 2048.

Run on the GPU box:   python tools/sparse_ab.py [--out profiles/sparse/ab.txt] [--quick]"""
import argparse, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_process_mpc_amd as g
from gaussian_process_mpc_amd.rollout import CostParams, GPPack, rollout
from gaussian_process_mpc_amd.synth import synth_problem

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--quick", action="store_true", help="small sizes only (a smoke run of the tool)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = g.require_gpu()
PEAK = 78.6e12
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def best_of(fns, reps=None):
    """{name: best seconds per call}; every call synchronised, candidates interleaved within a block."""
    reps = reps or args.reps
    best = {k: 1e9 for k in fns}
    for f in fns.values():
        f(); torch.cuda.synchronize()
    for _ in range(args.blocks):
        for k, f in fns.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                f(); torch.cuda.synchronize()
            best[k] = min(best[k], (time.perf_counter() - t0) / reps)
    return best


def problem(N, M, D=5, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (N, D))
    Y = np.sin(X).sum(axis=1, keepdims=True) + 0.05 * rng.standard_normal((N, 1))
    lam = rng.uniform(1.0, 3.0, D)
    Z = g.select_inducing(X[:min(N, 8192)], M, lam, method="random", seed=1)
    return torch.as_tensor(X, device=dev), torch.as_tensor(Y, device=dev), Z, lam


def torch_accumulate(st, X, Y, chunk):
    """Yardstick (a): the same mathematics, the chunk of k(Z, X_c) materialised, the products through torch.matmul."""
    il = torch.as_tensor(1.0 / st.lambdas, device=dev)
    Zs = st.Z * il.sqrt()
    kap = st.sigma_f ** 2 + st.noise_var
    G = torch.zeros((st.M, st.M), dtype=torch.float64, device=dev)
    r = torch.zeros((st.M, Y.shape[1]), dtype=torch.float64, device=dev)
    for n0 in range(0, X.shape[0], chunk):
        Xc = X[n0:n0 + chunk] * il.sqrt()
        K = st.sigma_f ** 2 * torch.exp(-0.5 * torch.cdist(Zs, Xc, compute_mode="donot_use_mm_for_euclid_dist") ** 2)
        V = st.W @ K
        Vw = V / (kap - (V * V).sum(dim=0))
        G += Vw @ V.T
        r += Vw @ Y[n0:n0 + chunk]
    return G, r


say("# sparse GP (FITC inducing points): tools/sparse_ab.py on one MI355X, best of %d blocks of %d synchronised calls" % (args.blocks, args.reps))
say("# 1. fit (gpmpc_sparse_accumulate, D = 5, one target, chunk 4096): ms per call, FMA and MFMA form | (a) torch.matmul on materialised chunks | (b) 3 N M^2 / 78.6 TFLOP/s")
L = g.lib()
default_form = L.gpmpc_sparse_set_form(-1)
say("# default form of this build: %s" % ("MFMA" if default_form else "FMA"))


def with_form(form, fn):
    def run():
        old = L.gpmpc_sparse_set_form(form)
        try:
            fn()
        finally:
            L.gpmpc_sparse_set_form(old)
    return run


for N in ((4096,) if args.quick else (4096, 32768, 262144)):
    for M in ((128,) if args.quick else (128, 512, 1024)):
        X, Y, Z, lam = problem(N, M)
        st = g.SparseGPState(Z, lam, 1.0, 0.05)
        b = best_of({"hip": with_form(0, lambda: st._accumulate(X, Y, 0)), "mfma": with_form(1, lambda: st._accumulate(X, Y, 0)),
                     "torch": lambda: torch_accumulate(st, X, Y, 4096)}, reps=1 if N * M * M > 1e10 else args.reps)
        Gt, rt = torch_accumulate(st, X, Y, 4096)
        st._accumulate(X, Y, 0)
        agree = float((st.G - Gt).abs().max() / Gt.abs().max())
        flops = 3.0 * N * M * M
        say("N %6d M %4d: FMA %9.3f ms (%5.2f TFLOP/s, %4.1f %% of peak)  MFMA %9.3f ms (%5.2f TFLOP/s, MFMA/FMA x%.2f) | (a) torch %9.3f ms "
            "(FMA/torch x%.2f, MFMA/torch x%.2f) | (b) %8.3f ms   [G agrees to %.1e]" %
            (N, M, b["hip"] * 1e3, flops / b["hip"] / 1e12, 100 * flops / b["hip"] / PEAK, b["mfma"] * 1e3, flops / b["mfma"] / 1e12,
             b["mfma"] / b["hip"], b["torch"] * 1e3, b["hip"] / b["torch"], b["mfma"] / b["torch"], flops / PEAK * 1e3, agree))
        del st, X, Y, Gt, rt
        torch.cuda.empty_cache()

say("# 2. append (rank one, six launches, no synchronisation inside) and refresh (torch inverse of B + gpmpc_sparse_finish): ms per call, 2 targets")
for M in ((32, 128) if args.quick else (32, 128, 256, 512, 1024)):
    X, Y, Z, lam = problem(4096, M)
    Y2 = torch.cat((Y, -Y), dim=1).contiguous()
    st = g.SparseGPState(Z, lam, 1.0, 0.05).fit(X, Y2)
    st.refresh_every = 0
    x, y = X[7].contiguous(), Y2[7].contiguous()
    b = best_of({"append": lambda: st.append(x, y), "refresh": lambda: st.refresh()}, reps=10)
    say("M %4d: append %7.3f ms   refresh %7.3f ms" % (M, b["append"] * 1e3, b["refresh"] * 1e3))

say("# 3. closed loop, data update + pack refill per step (ds 2, da 1; mean over 40 steps after 10 warm-up steps, synchronised per step)")


def loop_ms(dyn, pb, n0, steps=50, **kw):
    dyn.append_train_data(pb["X"][:n0, :2], pb["X"][:n0, 2:], pb["Y"][:n0])
    dyn.pack()
    ts = []
    for i in range(n0, n0 + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dyn.append_train_data(pb["X"][i, :2], pb["X"][i, 2:], pb["Y"][i], **kw)
        dyn.pack()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.mean(ts[10:]) * 1e3)


def with_hypers(dyn, pb):
    for gp in dyn.gpr_err:
        gp.set_lambdas(pb["lambdas"][0]); gp.set_sigma_n(np.array(0.05))
    return dyn


for N in ((400,) if args.quick else (400, 2000)):
    pb = synth_problem(7, N + 64, 2, 1, 5, 2)
    row = ["N %4d: dense incremental %7.3f ms" % (N, loop_ms(with_hypers(g.Dynamics(2, 1), pb), pb, N, incremental=True))]
    for M in (32, 128):
        Z = g.select_inducing(pb["X"][:N], M, pb["lambdas"][0])
        row.append("sparse M %3d %7.3f ms" % (M, loop_ms(with_hypers(g.SparseDynamics(2, 1, Z), pb), pb, N)))
    say("   ".join(row))

say("# 4. planner side, C3 shape (ds 4, da 1, H 20): solver callback (B = 1, host in / host out) and the B = 256 batch with gradient, ms per call")
if not args.quick:
    pb = synth_problem(3, 2048, 4, 1, 20, 256)
    dense = with_hypers(g.Dynamics(4, 1), pb)
    dense.append_train_data(pb["X"][:, :4], pb["X"][:, 4:], pb["Y"])
    sparse = with_hypers(g.SparseDynamics(4, 1, g.select_inducing(pb["X"], 256, pb["lambdas"][0])), pb)
    sparse.append_train_data(pb["X"][:, :4], pb["X"][:, 4:], pb["Y"])
    cost = CostParams(-1.0, pb["Q"], pb["R"])
    pd, ps = dense.pack(), sparse.pack()
    x0, U = torch.as_tensor(pb["x0"], device=dev), torch.as_tensor(pb["U"], device=dev)
    x0h, Uh = pb["x0"][0].copy(), pb["U"][0].copy()
    b = best_of({"cb_dense": lambda: pd.objective_gradient(x0h, Uh, cost), "cb_sparse": lambda: ps.objective_gradient(x0h, Uh, cost),
                 "b_dense": lambda: rollout(pd, x0, U, cost, want_traj=False), "b_sparse": lambda: rollout(ps, x0, U, cost, want_traj=False)}, reps=5)
    say("callback B = 1: dense N 2048 %8.3f ms | sparse M 256 %8.3f ms (x%.1f)     batch B = 256: dense %8.3f ms | sparse %8.3f ms (x%.1f)" %
        (b["cb_dense"] * 1e3, b["cb_sparse"] * 1e3, b["cb_dense"] / b["cb_sparse"], b["b_dense"] * 1e3, b["b_sparse"] * 1e3, b["b_dense"] / b["b_sparse"]))

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
