#!/usr/bin/env python3
"""Timings of the particle entry points on one MI355X against the ways the PARENT commit can produce the same numbers.

    python tools/particle_ab.py --out profiles/particles/ab.txt [--quick]

Per size: time per gp_posterior call and per particle-rollout step; the yardstick is torch on the kernel matrix of the existing
``gpmpc_predict(out_K=...)``: ``((Ks @ Kinv) * Ks).sum(-1)`` per GP (the parent's route to k*^T Kinv k* at many points).  Reported: the
ratios, the achieved TFLOP/s of the whole posterior call counted as 2 n^2 nq per matrix, the agreement between the routes, and the cost
of ``validate_plan(particles=4096)`` on the pendulum example next to one solve.  Best of ``--blocks`` blocks of ``--reps`` calls, one
synchronisation per block, after a warm-up (the method of tools/sparse_ab.py)."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_process_mpc_amd as G                                       # noqa: E402
from gaussian_process_mpc_amd._lib import check, host_doubles, lib, ptr, stream_ptr   # noqa: E402


def best_ms(fn, reps, blocks):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / reps)
    return 1e3 * best


def dense_model(n, ds, da, shared, seed=0):
    rng = np.random.default_rng(seed)
    D = ds + da
    X = torch.as_tensor(rng.uniform(-2, 2, (n, D)), device="cuda")
    lam = rng.uniform(2.0, 6.0, (ds, D))
    if shared:
        lam = np.tile(lam[:1], (ds, 1))
    sf = np.ones(ds)
    Y = torch.as_tensor(rng.standard_normal((n, ds)), device="cuda")
    Ks = []
    for a in range(1 if shared else ds):
        Ky = torch.empty((n, n), dtype=torch.float64, device="cuda")
        check(lib().gpmpc_build_ky(n, D, ptr(X), host_doubles(lam[a])[1], 1.0, 1e-2, None, ptr(Ky), stream_ptr()), "gpmpc_build_ky")
        Ks.append(torch.linalg.inv(Ky))
    Kinv = Ks[0] if shared else torch.stack(Ks)
    beta = torch.stack([(Ks[0] if shared else Ks[a]) @ Y[:, a] for a in range(ds)], dim=1)
    return G.GPModel(X, beta, Kinv, lam, sf, ds, da)


def torch_route(model, Z):
    """The parent's route: K* from gpmpc_predict(out_K), then ((K* @ Kinv) * K*).sum(-1) and K* @ beta per GP."""
    nq, n, D = Z.shape[0], model.n, model.D
    K = torch.empty((nq, n), dtype=torch.float64, device="cuda")
    nb = lib().gpmpc_predict_workspace_bytes(n, D, nq)
    ws = torch.empty(max(int(nb), 256), dtype=torch.uint8, device="cuda")
    means, vars_ = [], []
    shared = model.Kinv.dim() == 2
    same_hyper = shared and all(np.array_equal(model.lambdas[a], model.lambdas[0]) for a in range(model.ds))
    q = None
    for a in range(model.ds):
        if a == 0 or not same_hyper:
            check(lib().gpmpc_predict(n, D, ptr(model.X), host_doubles(model.lambdas[a])[1], float(model.sigma_f[a]), None, None, 0.0, nq, ptr(Z),
                                      ptr(K), None, None, ctypes.c_void_p(ws.data_ptr()), nb, stream_ptr()), "gpmpc_predict")
            Ka = model.Kinv if shared else model.Kinv[a]
            q = ((K @ Ka.T) * K).sum(-1)
        means.append(K @ model.beta[:, a])
        vars_.append(float(model.sigma_f[a]) ** 2 - q)
    return torch.stack(means, dim=1), torch.stack(vars_, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--no-pendulum", action="store_true")
    a = ap.parse_args()
    G.require_gpu()
    lines = ["# tools/particle_ab.py on %s: best of %d blocks of %d calls, one synchronisation per block" % (torch.cuda.get_device_name(0), a.blocks, a.reps)]
    sizes = [("N=300 ds=4 per-GP", 300, 4, 1, False, 256 * 64), ("N=2048 ds=4 per-GP", 2048, 4, 1, False, 4096),
             ("N=2048 ds=4 shared", 2048, 4, 1, True, 4096), ("M=256 ds=4 shared (a sparse model's shape)", 256, 4, 1, True, 4096)]
    if a.quick:
        sizes = [("N=300 ds=4 per-GP", 300, 4, 1, False, 1024)]
    for name, n, ds, da, shared, nq in sizes:
        model = dense_model(n, ds, da, shared)
        Z = torch.as_tensor(np.random.default_rng(1).uniform(-2, 2, (nq, ds + da)), device="cuda")
        t_new = best_ms(lambda: G.gp_posterior(model, Z), a.reps, a.blocks)
        t_old = best_ms(lambda: torch_route(model, Z), a.reps, a.blocks)
        m1, v1 = G.gp_posterior(model, Z)
        m0, v0 = torch_route(model, Z)
        mats = 1 if shared else ds
        tflops = 2.0 * n * n * nq * mats / (t_new * 1e-3) / 1e12
        # one rollout step: B x P = nq columns
        P = min(nq, 4096)
        Bp = nq // P
        x = Z[:, :ds].reshape(Bp, P, ds).contiguous()
        U = torch.zeros((Bp, da), dtype=torch.float64, device="cuda")
        eps = G.particle_noise(P, da + ds, 1, 0, 0)
        t_step = best_ms(lambda: G.particle_step(model, x, U, eps), a.reps, a.blocks)
        lines.append("%-44s nq %6d | gp_posterior %8.3f ms (%.2f TFLOP/s over 2 n^2 nq x %d matrices) | torch on gpmpc_predict's K* %8.3f ms | "
                     "ratio new/old %.2f | rollout step (B %d x P %d) %8.3f ms | agreement: mean %.1e, var %.1e (max abs)"
                     % (name, nq, t_new, tflops, mats, t_old, t_new / t_old, Bp, P, t_step, float((m1 - m0).abs().max()), float((v1 - v0).abs().max())))
        print(lines[-1], flush=True)
        del model
    if not a.no_pendulum and not a.quick:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
        import particle_validation as PV
        mpc, x0 = PV.pendulum_mpc(prob=0.95, inducing=0)
        t0 = time.perf_counter()
        mpc.get_optimal_trajectory(x0)
        torch.cuda.synchronize()
        t_solve = time.perf_counter() - t0
        mpc.validate_plan(particles=4096)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mpc.validate_plan(particles=4096)
        torch.cuda.synchronize()
        t_val = time.perf_counter() - t0
        lines.append("pendulum example: one solve (%s) %.1f ms | validate_plan(particles=4096) %.1f ms" % (mpc.solver_used, 1e3 * t_solve, 1e3 * t_val))
        print(lines[-1], flush=True)
    lines.append("# not measured: hardware counters of the new kernels, sizes above N = 4096, multi-GPU")
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
