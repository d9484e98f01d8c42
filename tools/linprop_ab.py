#!/usr/bin/env python3
"""Timings of the linearised rollout on one MI355X against the moment-matched rollout of the SAME build on the same data.

    python tools/linprop_ab.py --out profiles/linprop/ab.txt [--quick]

``rollout`` is unchanged code, hence the parent's: the ratio linearised / moment-matched per shape is the A/B, objective only and with
gradient.  No ratio is fixed in advance; a shape where the linearised form is SLOWER is reported like any other.  Method (the measuring
guide of the project): a warm-up call, then ``--blocks`` timed blocks of ``--reps`` calls with one synchronisation per block; reported are
the median block and the spread (min ... max) of the blocks, in ms per call.  The two rules do not compute the same numbers (one is exact
moment matching, the other its first-order approximation): the last column is how far apart their costs are on the measured (random)
plans, for orientation only.

    python tools/linprop_ab.py --form all --out profiles/linprop/stream_ab.txt

``--form`` measures the forms of the linearised step (gpmpc_linearised_set_form) by the same protocol on the grid B = 1 ... 256 of the four
shapes: ``all`` prints TILE | STREAM | moment matching per row, the ratios STREAM / TILE and STREAM / moment matching, and at B = 1 the
Kinv bandwidth STREAM reaches per step (bytes of the matrices it streams per step over its time per step); ``tile``, ``stream`` or ``auto``
times that form alone (the parent's TILE timing is taken with the parent's build of this tool's first table or a script like it)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_process_mpc_amd as G                                       # noqa: E402
from gaussian_process_mpc_amd._lib import check, host_doubles, lib, ptr, stream_ptr   # noqa: E402


def blocks_ms(fn, reps, blocks):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def models(n, ds, da, shared, seed=0):
    """The same GP bundle as a GPModel (linearised) and as a GPPack (moment matching)."""
    rng = np.random.default_rng(seed)
    D = ds + da
    X = torch.as_tensor(rng.uniform(-2, 2, (n, D)), device="cuda")
    lam = rng.uniform(2.0, 6.0, (ds, D))
    if shared:
        lam = np.tile(lam[:1], (ds, 1))
    sf = np.ones(ds)
    Y = torch.as_tensor(np.sin(X.cpu().numpy() @ rng.standard_normal((D, ds))) + 0.1 * rng.standard_normal((n, ds)), device="cuda")
    Ks = []
    for a in range(1 if shared else ds):
        Ky = torch.empty((n, n), dtype=torch.float64, device="cuda")
        check(lib().gpmpc_build_ky(n, D, ptr(X), host_doubles(lam[a])[1], 1.0, 1e-2, None, ptr(Ky), stream_ptr()), "gpmpc_build_ky")
        Ks.append(torch.linalg.inv(Ky))
    Kinv = Ks[0] if shared else torch.stack(Ks)
    beta = torch.stack([(Ks[0] if shared else Ks[a]) @ Y[:, a] for a in range(ds)], dim=1)
    return G.GPModel(X, beta, Kinv, lam, sf, ds, da), G.GPPack(X, Y, Kinv, lam, sf)


def sparse_models(M, ds, da, n_obs=2048, seed=0):
    """A FITC model of M inducing points fed n_obs observations (SparseDynamics): its (Z, alpha, Q) through GPModel.from_dynamics, and the
    pack its own rollout uses.  One hyper-parameter set for all GPs, so Q is ONE matrix."""
    rng = np.random.default_rng(seed)
    D = ds + da
    X = rng.uniform(-2, 2, (n_obs, D))
    Y = np.sin(X @ rng.standard_normal((D, ds))) + 0.1 * rng.standard_normal((n_obs, ds))
    dyn = G.SparseDynamics(ds, da, X[rng.choice(n_obs, size=M, replace=False)])
    lam = rng.uniform(2.0, 6.0, D)
    for g in dyn.gpr_err:
        g.set_lambdas(lam)
        g.set_sigma_f(1.0)
        g.set_sigma_n(0.1)
    dyn.append_train_data(X[:, :ds], X[:, ds:], Y)
    return G.GPModel.from_dynamics(dyn), dyn.pack(), dyn


def fmt(t):
    return "%9.3f (%.3f ... %.3f)" % t


FORM_BATCHES = (1, 2, 4, 8, 16, 32, 64, 256)


def form_table(a, lines, save):
    """The grid of --form: per shape and B, ms per call of every requested form and of the moment-matched rollout."""
    H, ds, da = 20, 4, 1
    forms = ("tile", "stream") if a.form == "all" else (a.form,)
    shapes = [("N=2048 ds=4 per-GP Kinv", 2048, False), ("N=2048 ds=4 shared Kinv", 2048, True), ("N=300 ds=4 per-GP Kinv", 300, False),
              ("M=256 ds=4 SparseDynamics (FITC, 2048 observations)", 256, None)]
    batches = FORM_BATCHES
    if a.quick:
        shapes, batches = shapes[2:3], (1, 16)
    cost = G.CostParams(-1.0, np.eye(ds), 0.1 * np.eye(da))
    rng = np.random.default_rng(1)
    lines.append("# forms of the linearised step: %s; columns per mode: %s | moment matching" % (", ".join(forms), " | ".join(forms)))
    for name, n, shared in shapes:
        keep = None
        if shared is None:
            gm, pack, keep = sparse_models(n, ds, da)
        else:
            gm, pack = models(n, ds, da, shared)
        nmat = 1 if gm.c.gp_stride == 0 else ds
        for B in batches:
            x0 = torch.as_tensor(rng.uniform(-1, 1, (B, ds)), device="cuda")
            U = torch.as_tensor(rng.uniform(-1, 1, (B, H, da)), device="cuda")
            t = {}
            for grad in (False, True):
                for f in forms:
                    t[f, grad] = blocks_ms(lambda: G.linearised_rollout(gm, x0, U, cost, want_grad=grad, want_traj=False, form=f), a.reps, a.blocks)
                t["mm", grad] = blocks_ms(lambda: G.rollout(pack, x0, U, cost, want_grad=grad, want_traj=False), a.reps, a.blocks)
            txt = "%-52s B %4d" % (name, B)
            for grad, label in ((False, "objective"), (True, "with gradient")):
                txt += " | %s: " % label + " ".join("%s %s" % (f, fmt(t[f, grad])) for f in forms) + " moment matching %s" % fmt(t["mm", grad])
                if a.form == "all":
                    txt += " stream/tile %.3f stream/mm %.3f" % (t["stream", grad][0] / t["tile", grad][0], t["stream", grad][0] / t["mm", grad][0])
            if "stream" in forms and B == 1:
                # one pass over every matrix per step at B = 1 (ds <= GPMPC_LINPROP_STREAM_COLS): bytes of Kinv over the time of a step
                gb = nmat * float(gm.n) * gm.n * 8 / 1e9
                txt += " | STREAM Kinv stream per step %.1f MB: %.2f TB/s objective, %.2f TB/s with gradient (whole call / H, launches and tail included)" % (
                    1e3 * gb, gb / (t["stream", False][0] / H), gb / (t["stream", True][0] / H))
            lines.append(txt)
            print(txt, flush=True)
            save()
        del gm, pack, keep
        torch.cuda.empty_cache()


def bits_table(a):
    """--bits: a SHA-256 of every output of the entries that take a model (and of the pack MPPI solves) at small ragged shapes, one line
    each.  Run once per library (GPMPC_LIB_PATH) and compare the two files: a host refactor must leave every line as it was.
    N = 70 (one full and one ragged 64-row block, 128 padded rows, eight k-stages), ds = 2, da = 1, B = 65 columns (one full and one ragged
    tile), H = 3; per-GP and shared Kinv, the two GPs in one (lambda, sigma_f) group and in two."""
    import hashlib
    n, ds, da, B, H, K = 70, 2, 1, 65, 3, 8
    rng = np.random.default_rng(7)
    x0 = torch.as_tensor(rng.uniform(-1, 1, (B, ds)), device="cuda")
    U = torch.as_tensor(rng.uniform(-1, 1, (B, H, da)), device="cuda")
    Z = torch.as_tensor(rng.uniform(-1, 1, (B, ds + da)), device="cuda")
    cost = G.CostParams(-1.0, np.eye(ds), 0.1 * np.eye(da))
    rows = G.StateConstraints(np.array([[1.0, 0.0], [0.0, -1.0]]), np.array([0.8, 0.9]), 1.0)
    lines = []

    def put(name, t):
        t = t if isinstance(t, np.ndarray) else t.detach().cpu().contiguous().numpy()
        lines.append("%-64s %s %s" % (name, "x".join(map(str, t.shape)), hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest()))

    for shared in (False, True):
        for one_group in (False, True):
            gm, pack = models(n, ds, da, one_group)
            if shared != one_group:                      # the other pairing of matrices and groups: the model's arrays, regrouped
                Kinv = gm.Kinv[0].contiguous() if shared else torch.stack([gm.Kinv, gm.Kinv])
                gm = G.GPModel(gm.X, gm.beta, Kinv, gm.lambdas, gm.sigma_f, ds, da)
            tag = "%s Kinv, %d group%s: " % ("shared" if shared else "per-GP", 1 if one_group else 2, "" if one_group else "s")
            for k, t in zip(("mean", "var"), G.gp_posterior(gm, Z)):
                put(tag + "gp_posterior " + k, t)
            r = G.particle_rollout(gm, x0, U, particles=8, seed=3, constraints=rows)
            for k in ("particles", "mean", "cov", "clamped", "violation", "joint_violation"):
                put(tag + "particle_rollout P=8 " + k, r[k])
            for form in ("tile", "stream"):
                r = G.linearised_rollout(gm, x0, U, cost, want_grad=True, want_jac=True, constraints=rows, form=form)
                for k in ("cost", "grad", "means", "vars", "jac", "g", "g_jac"):
                    put(tag + "linearised_rollout %s %s" % (form, k), r[k])
            r = G.linearised_rollout(gm, x0, U, cost, want_grad=True, want_jac=True, constraints=rows, full_covariance=True)
            for k in ("cost", "grad", "means", "covs", "jac", "g", "g_jac"):
                put(tag + "linearised_fc_rollout " + k, r[k])
            kw = dict(samples=K, iterations=3, sigma=0.5, lb=-2.0, ub=2.0, seed=5)
            for cons in (None, rows):
                solves = [("mppi_solve_linearised", lambda: G.mppi_solve_linearised(gm, x0[0], U[0], cost, constraints=cons, **kw)),
                          ("mppi_solve_particles P=8", lambda: G.mppi_solve_particles(gm, x0[0], U[0], cost, constraints=cons, particles=8, **kw))]
                if shared == one_group:                  # (the pack solves do not see the regrouped model: once per pack)
                    solves += [("mppi_solve", lambda: G.mppi_solve(pack, x0[0], U[0], cost, constraints=cons, **kw)),
                               ("mppi_solve_fullcov", lambda: G.mppi_solve(pack, x0[0], U[0], cost, constraints=cons, full_covariance=True, **kw))]
                for name, solve in solves:
                    s = solve()
                    for k in ("U", "trace"):
                        put(tag + "%s rows=%d %s" % (name, 0 if cons is None else 2, k), s[k])
                    put(tag + "%s rows=%d key" % (name, 0 if cons is None else 2), np.array([s["violation"], s["cost"]]))
            del gm, pack
    torch.cuda.synchronize()
    out = "\n".join(lines) + "\n"
    if a.bits != "-":
        os.makedirs(os.path.dirname(a.bits) or ".", exist_ok=True)
        with open(a.bits, "w") as f:
            f.write(out)
    print(out, end="")
    print("# %d outputs hashed" % len(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--bits", default=None, metavar="FILE", help="write a SHA-256 of every model-entry output at small ragged shapes and stop")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--form", choices=("tile", "stream", "auto", "all"), default=None,
                    help="measure the forms of the linearised step on the grid B = 1 ... 256 (all: TILE | STREAM | moment matching)")
    a = ap.parse_args()
    G.require_gpu()
    if a.bits:
        return bits_table(a)
    lines = ["# tools/linprop_ab.py on %s: ms per call, median block (min ... max) of %d blocks of %d calls after a warm-up; H = 20, da = 1"
             % (torch.cuda.get_device_name(0), a.blocks, a.reps)]
    H, ds, da = 20, 4, 1

    def save():                                          # after every line: a run that is cut short leaves what it measured
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    if a.form:
        form_table(a, lines, save)
        lines.append("# not measured: hardware counters of the new kernels, sizes above N = 2048, other ds / da, B above 256, multi-GPU")
        save()
        return
    shapes = [("N=2048 ds=4 per-GP Kinv", 2048, False, (1, 16, 256, 4096)), ("N=2048 ds=4 shared Kinv", 2048, True, (1, 16, 256, 4096)),
              ("N=300 ds=4 per-GP Kinv", 300, False, (256,)), ("M=256 ds=4 SparseDynamics (FITC, 2048 observations)", 256, None, (256,))]
    if a.quick:
        shapes = [("N=300 ds=4 per-GP Kinv", 300, False, (16,))]
    cost = G.CostParams(-1.0, np.eye(ds), 0.1 * np.eye(da))
    rng = np.random.default_rng(1)
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
            row = []
            for grad in (False, True):
                t_lin = blocks_ms(lambda: G.linearised_rollout(gm, x0, U, cost, want_grad=grad, want_traj=False), reps, a.blocks)
                t_mm = blocks_ms(lambda: G.rollout(pack, x0, U, cost, want_grad=grad, want_traj=False), reps, a.blocks)
                row.append((t_lin, t_mm))
            c_lin = G.linearised_rollout(gm, x0, U, cost, want_grad=False, want_traj=False)["cost"]
            c_mm = G.rollout(pack, x0, U, cost, want_grad=False, want_traj=False)["cost"]
            both = torch.isfinite(c_lin) & torch.isfinite(c_mm)                    # (gamma < 0: a plan far from the data can leave either cost NaN)
            rel = float(((c_lin - c_mm).abs() / c_mm.abs())[both].median()) if bool(both.any()) else float("nan")
            lines.append("%-44s B %5d | objective: linearised %s moment matching %s ratio %.3f | with gradient: linearised %s moment matching %s "
                         "ratio %.3f | plans/s linearised %.0f (objective) | median relative cost difference between the rules %.2e (%d of %d plans finite under both)"
                         % (name, B, fmt(row[0][0]), fmt(row[0][1]), row[0][0][0] / row[0][1][0], fmt(row[1][0]), fmt(row[1][1]),
                            row[1][0][0] / row[1][1][0], B / (row[0][0][0] * 1e-3), rel, int(both.sum()), B))
            print(lines[-1], flush=True)
            save()
        if n == 2048 and not a.quick:
            K, iters = 1024, 5
            x0 = rng.uniform(-1, 1, ds)
            U0 = np.zeros((H, da))
            kw = dict(samples=K, iterations=iters, sigma=0.5, lb=-2.0, ub=2.0, seed=1)
            t_lin = blocks_ms(lambda: G.mppi_solve_linearised(gm, x0, U0, cost, **kw), 1, a.blocks)
            t_mm = blocks_ms(lambda: G.mppi_solve(pack, x0, U0, cost, **kw), 1, a.blocks)
            lines.append("%-44s one MPPI solve, %d samples x %d iterations | linearised %s moment matching %s ratio %.3f"
                         % (name, K, iters, fmt(t_lin), fmt(t_mm), t_lin[0] / t_mm[0]))
            print(lines[-1], flush=True)
            save()
        del gm, pack, keep
        torch.cuda.empty_cache()
    lines.append("# not measured: hardware counters of the new kernels, sizes above N = 2048, other ds / da, multi-GPU")
    save()


if __name__ == "__main__":
    main()
