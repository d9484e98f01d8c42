"""Holds tests/particle_reference.py itself and everything of the particle entry points that needs no device (CPU):

  * the C ABI: names, signatures, the layout of gpmpc_gp_model against the header, workspace sizes, every refusal before any launch;
  * the pointwise posterior of the reference IS the oracle's moment matching at S = 0 (an exact identity), to 1e-12 relative;
  * the statistical pin of the semantics: at step 1 the reference's particle mean and variance agree with the oracle's exact moment
    matching within 4 Monte-Carlo standard errors per entry (P = 4096, a fixed seed) -- plain, with a nominal model, with process_var;
  * noise addressing: a value does not change with B or P, plans share draws; a zero pivot in init_cov."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import particle_reference as R
from oracle import gpmpc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gpmpc_gp_posterior_workspace_bytes", "gpmpc_gp_posterior", "gpmpc_particle_noise", "gpmpc_particle_step_workspace_bytes",
         "gpmpc_particle_step", "gpmpc_particle_stats", "gpmpc_particle_rollout_workspace_bytes", "gpmpc_particle_rollout"]
E_ARG, E_WORKSPACE = -1, -4


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_mpc_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_abi_names_and_signatures(L):
    from gaussian_process_mpc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        res, args = _lib.SIGNATURES[name]
        assert res in (ctypes.c_int, ctypes.c_size_t)
        assert getattr(L, name) is not None
        n_decl = len(re.search(r"\b%s\s*\((.*?)\);" % name, hdr, flags=re.S).group(1).split(","))
        assert n_decl == len(args), (name, n_decl, len(args))
    import gaussian_process_mpc_amd as g
    for name in ("GPModel", "gp_posterior", "particle_noise", "particle_step", "particle_stats", "particle_rollout"):
        assert hasattr(g, name)
    assert hasattr(g.Dynamics, "particle_rollout") and hasattr(g.SparseDynamics, "particle_rollout") and hasattr(g.RiskSensitiveMPC, "validate_plan")


def test_gp_model_struct_layout_matches_header(L, tmp_path):
    from gaussian_process_mpc_amd._lib import GPModelC
    names = [f[0] for f in GPModelC._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpmpc.h"\nint main(){printf("%zu"' + ' " %zu"' * len(names)
                   + ', sizeof(gpmpc_gp_model), ' + ", ".join("offsetof(gpmpc_gp_model,%s)" % n for n in names) + ');return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(GPModelC)
    assert out[1:] == [getattr(GPModelC, n).offset for n in names]
    assert names == ["n", "state_dim", "action_dim", "has_nominal", "has_noise", "reserved", "X", "beta", "Kinv", "ld", "gp_stride", "lambdas",
                     "sigma_f", "nom_w", "nom_b", "init_cov", "action_var", "process_var"]


def _model_c(n=10, ds=2, da=1, ld=None, gp_stride=0, X=4096, beta=4096, Kinv=4096, lam=1.0, sf=1.0, nominal=None, init_cov=None,
             action_var=None, process_var=None):
    """A gpmpc_gp_model whose device pointers are never dereferenced: every call it travels in is refused first."""
    from gaussian_process_mpc_amd._lib import GPModelC
    c = GPModelC()
    D = ds + da
    c.n, c.state_dim, c.action_dim = n, ds, da
    c.X, c.beta, c.Kinv = X, beta, Kinv
    c.ld, c.gp_stride = (n if ld is None else ld), gp_stride
    for k in range(min(max(ds * D, 0), 64)):
        c.lambdas[k] = lam
    for k in range(min(max(ds, 0), 8)):
        c.sigma_f[k] = sf
    if nominal is not None:
        c.has_nominal = 1
        c.nom_w[0] = nominal
    if init_cov is not None or action_var is not None or process_var is not None:
        c.has_noise = 1
        P = np.eye(ds) * 1e-3 if init_cov is None else np.asarray(init_cov, dtype=np.float64)
        c.init_cov[:ds * ds] = P.reshape(-1).tolist()
        c.action_var[:da] = [1e-3 if action_var is None else action_var] * da
        c.process_var[:ds] = [0.0 if process_var is None else process_var] * ds
    return c


MODEL_REFUSALS = {
    "state_dim": dict(ds=0), "state_dim = 9": dict(ds=9, da=0), "action_dim": dict(ds=8, da=1), "action_dim = -1": dict(da=-1), "n < 1": dict(n=0),
    "ld < n": dict(ld=9), "NULL pointer": dict(X=None), "NULL pointer (model arrays)": dict(Kinv=None), "NULL": dict(beta=None),
    "lambdas": dict(lam=0.0), "lambdas[0][0] = nan": dict(lam=float("nan")), "sigma_f": dict(sf=-1.0), "nominal": dict(nominal=float("inf")),
    "init_cov holds a non-finite": dict(init_cov=[[1.0, 0.0], [0.0, float("nan")]]),
    "init_cov is not symmetric": dict(init_cov=[[1.0, 0.1], [0.2, 1.0]]),
    "negative pivot": dict(init_cov=[[1.0, 2.0], [2.0, 1.0]]), "negative pivot (": dict(init_cov=[[-1.0, 0.0], [0.0, 1.0]]),
    "action_var": dict(action_var=-1e-3), "process_var": dict(process_var=-1.0), "process_var[0] = inf": dict(process_var=float("inf")),
}


def test_refusals_before_any_launch(L):
    """Every refusal is decided on the host, from sizes, pointers and the host parts of the model: GPMPC_E_ARG with a text (no device is
    touched: this runs without one)."""
    from gaussian_process_mpc_amd._lib import StateConstraintsC
    p = ctypes.c_void_p(4096)
    big = 1 << 40
    ok = _model_c()

    def post(m=ok, nq=5, z=p, mean=p, var=p, chunk=64, ws=p, nb=big):
        return L.gpmpc_gp_posterior(ctypes.byref(m) if m is not None else None, nq, z, mean, var, chunk, ws, nb, None)

    def step(m=ok, B=2, P=3, x=p, U=p, us=1, eps=p, nxt=p, chunk=64, ws=p, nb=big):
        return L.gpmpc_particle_step(ctypes.byref(m), B, P, x, U, us, eps, nxt, None, None, chunk, ws, nb, None)

    cons = StateConstraintsC()
    cons.n_rows = 1

    def roll(m=ok, B=2, P=3, H=2, x0=p, U=p, cons=None, part=p, mean=p, cov=p, cl=p, viol=None, joint=None, chunk=64, ws=p, nb=big):
        return L.gpmpc_particle_rollout(ctypes.byref(m), B, P, H, x0, U, 1, 0, ctypes.byref(cons) if cons is not None else None, part, mean, cov,
                                        cl, viol, joint, chunk, ws, nb, None)

    def stats(B=2, P=3, T=2, ds=2, part=p, var=None, cons=None, mean=p, cov=p, cl=None, viol=None, joint=None):
        return L.gpmpc_particle_stats(B, P, T, ds, part, var, ctypes.byref(cons) if cons is not None else None, mean, cov, cl, viol, joint, None)

    def refused(rc, text, who):
        msg = L.gpmpc_last_error().decode()
        assert rc == E_ARG and text in msg and who in msg, (rc, text, msg)

    for text, kw in MODEL_REFUSALS.items():                   # the model, through every entry point that takes one
        bad = _model_c(**kw)
        refused(post(m=bad), text, "gpmpc_gp_posterior")
        refused(step(m=bad), text, "gpmpc_particle_step")
        refused(roll(m=bad), text, "gpmpc_particle_rollout")
    refused(post(m=None), "NULL pointer", "gpmpc_gp_posterior")
    for text, kw in {"nq < 1": dict(nq=0), "chunk": dict(chunk=96), "chunk must": dict(chunk=-64), "NULL pointer": dict(z=None), "NULL": dict(var=None),
                     "NULL p": dict(ws=None)}.items():
        refused(post(**kw), text, "gpmpc_gp_posterior")
    assert post(nb=L.gpmpc_gp_posterior_workspace_bytes(ctypes.byref(ok), 5, 64) - 1) == E_WORKSPACE
    for text, kw in {"B < 1": dict(B=0), "P < 1": dict(P=0), "chunk": dict(chunk=100), "NULL pointer": dict(x=None), "NULL": dict(U=None),
                     "NULL p": dict(eps=None), "NULL po": dict(nxt=None), "u_stride": dict(us=0), "2^31": dict(B=1 << 16, P=1 << 16)}.items():
        refused(step(**kw), text, "gpmpc_particle_step")
    assert step(nb=L.gpmpc_particle_step_workspace_bytes(ctypes.byref(ok), 2, 3, 64) - 1) == E_WORKSPACE
    bad_rows, nan_kappa = StateConstraintsC(), StateConstraintsC()
    bad_rows.n_rows, nan_kappa.n_rows = 17, 1
    nan_kappa.kappa[0] = float("nan")
    for text, kw in {"H < 1": dict(H=0), "B < 1": dict(B=0), "P < 1": dict(P=0), "chunk": dict(chunk=32), "NULL pointer": dict(x0=None),
                     "NULL": dict(U=None), "NULL p": dict(part=None), "NULL po": dict(cl=None), "n_rows": dict(cons=bad_rows, viol=p, joint=p),
                     "kappa": dict(cons=nan_kappa, viol=p, joint=p), "exactly when": dict(cons=cons, viol=p), "exactly": dict(viol=p)}.items():
        refused(roll(**kw), text, "gpmpc_particle_rollout")
    assert roll(nb=L.gpmpc_particle_rollout_workspace_bytes(ctypes.byref(ok), 2, 3, 2, 64) - 1) == E_WORKSPACE
    for text, kw in {"state_dim": dict(ds=0), "state_dim = 9": dict(ds=9), "B < 1": dict(B=0), "P < 1": dict(P=0), "T (steps)": dict(T=0),
                     "NULL pointer": dict(part=None), "given together": dict(var=p), "n_rows": dict(cons=bad_rows, viol=p, joint=p),
                     "exactly when": dict(cons=cons, joint=p)}.items():
        refused(stats(**kw), text, "gpmpc_particle_stats")
    for text, args in {"P < 1": (0, 3, 0), "n_normals": (4, 0, 0), "n_normals = 17": (4, 17, 0), "t < 0": (4, 3, -1)}.items():
        refused(L.gpmpc_particle_noise(args[0], args[1], args[2], 1, 0, p, None), text, "gpmpc_particle_noise")
    refused(L.gpmpc_particle_noise(4, 3, 0, 1, 0, None, None), "NULL pointer", "gpmpc_particle_noise")


def test_workspace_sizes(L):
    m = _model_c(n=70, ds=2, da=1)
    post = lambda nq, chunk, mm=m: L.gpmpc_gp_posterior_workspace_bytes(ctypes.byref(mm), nq, chunk)  # noqa: E731
    assert post(200, 64) == post(10 ** 6, 64)                              # the chunk bounds it
    assert post(200, 0) == post(200, 4096) and post(10 ** 6, 0) == post(10 ** 6, 4096)
    assert post(200, 64) >= 8 * (128 * 64 + 2 * 64 + 2 * 2 * 64)           # Ks (n padded to 128), two row blocks of partial sums for m and for q
    assert post(200, 100) == 0 and post(0, 64) == 0 and post(200, -64) == 0
    step, roll = L.gpmpc_particle_step_workspace_bytes, L.gpmpc_particle_rollout_workspace_bytes
    assert step(ctypes.byref(m), 2, 70, 64) >= post(140, 64) + 8 * 140 * 3
    assert roll(ctypes.byref(m), 2, 70, 3, 64) >= step(ctypes.byref(m), 2, 70, 64) + 8 * (70 * 3 + 3 * 140 * 2)
    assert step(ctypes.byref(m), 0, 70, 64) == 0 and roll(ctypes.byref(m), 2, 70, 0, 64) == 0


# ------------------------------------------------------------------------------------------------------------------ semantics
@functools.lru_cache(maxsize=None)
def _pin_problem():
    """ds = 2, da = 1, N = 48, per-GP lambda, sf != 1; Kinv = inv(Ky) in float64 (data, as a caller would hand it over)."""
    rng = np.random.default_rng(11)
    n, ds, da = 48, 2, 1
    X = rng.uniform(-1.5, 1.5, (n, ds + da))
    lam = np.array([[1.1, 1.7, 2.3], [2.0, 0.9, 1.4]])
    sf = np.array([1.3, 0.8])
    sn = np.array([0.1, 0.12])
    Y = np.stack([np.sin(X[:, 0]) + 0.5 * X[:, 2] + 0.3 * X[:, 1] ** 2, np.cos(X[:, 1]) * X[:, 0] - 0.4 * X[:, 2]], axis=1)
    Y = Y + sn[None, :] * rng.standard_normal((n, ds))
    return dict(X=X, Y=Y, lam=lam, sf=sf, sn=sn, x0=np.array([0.3, -0.2]), u0=np.array([0.4]))


def _pin_model(nominal=None, process_var=None):
    pb = _pin_problem()
    X, Y = pb["X"], pb["Y"]
    if nominal is not None:
        Y = Y - X @ nominal[0].T - nominal[1]
    Kinv = np.stack([np.linalg.inv(O.kernel_matrices(torch.as_tensor(X), torch.as_tensor(pb["lam"][a]), float(pb["sf"][a]), float(pb["sn"][a]))[1].numpy())
                     for a in range(2)])
    beta = np.stack([Kinv[a] @ Y[:, a] for a in range(2)], axis=1)
    m = dict(X=X, beta=beta, Kinv=Kinv, lam=pb["lam"], sf=pb["sf"], init_cov=np.diag([0.05, 0.02]), action_var=np.array([0.01]), Yres=Y)
    if nominal is not None:
        m["nominal"] = nominal
    if process_var is not None:
        m["process_var"] = process_var
    return m


def _oracle_moments(model, u, S):
    """Exact moment matching of one step at input N(u, S): mean and variance per GP from the oracle, plus -- exact for a linear model --
    the nominal terms mu += W u + b, var += W S W^T + 2 W S dmu/du, and process_var."""
    ds = 2
    ut = torch.tensor(u, dtype=torch.float64, requires_grad=True)
    St = torch.as_tensor(S)
    mu, var = np.empty(ds), np.empty(ds)
    for a in range(ds):
        Ki, lam, y = torch.as_tensor(model["Kinv"][a]), torch.as_tensor(model["lam"][a]), torch.as_tensor(model["Yres"][:, a])
        m, beta, _ = O.mean_prop(Ki, lam, ut, St, torch.as_tensor(model["X"]), y, float(model["sf"][a]))
        v = O.variance_prop(Ki, lam, ut, St, torch.as_tensor(model["X"]), m, beta, float(model["sf"][a]))
        (dm,) = torch.autograd.grad(m, ut)
        mu[a], var[a] = float(m.detach()), float(v.detach())
        if "nominal" in model:
            W, b = model["nominal"]
            mu[a] += W[a] @ u + b[a]
            var[a] += W[a] @ S @ W[a] + 2.0 * W[a] @ S @ dm.numpy()
        if "process_var" in model:
            var[a] += model["process_var"][a]
    return mu, var


def test_posterior_is_moment_matching_at_zero_input_covariance():
    """S = 0 collapses exact moment matching to the pointwise posterior: m = beta . k, var = sf^2 - k^T Kinv k (an exact identity)."""
    m = _pin_model()
    rng = np.random.default_rng(2)
    Z = rng.uniform(-1.0, 1.0, (6, 3))
    r = R.posterior(m, Z)
    for c in range(Z.shape[0]):
        mu, var = _oracle_moments(m, Z[c], np.zeros((3, 3)))
        em = np.abs(R.G.to_f64(r["m"][c]) - mu) / R.G.to_f64(r["m_abs"][c])
        ev = np.abs(R.G.to_f64(r["s2"][c]) - var) / (m["sf"] ** 2 + R.G.to_f64(r["q_abs"][c]))
        print("  point %d: mean %.2e, variance %.2e relative" % (c, em.max(), ev.max()))
        assert em.max() <= 1e-12 and ev.max() <= 1e-12


NOMINAL = (np.array([[0.9, 0.05, 0.1], [-0.1, 0.8, 0.2]]), np.array([0.02, -0.03]))


@pytest.mark.parametrize("variant", ["plain", "nominal", "process_var"])
def test_step_one_agrees_with_moment_matching_within_four_standard_errors(variant):
    """The statistical pin of the semantics: P = 4096 particles of the reference, seed 1, step 1, input covariance diag(0.05, 0.02, 0.01)."""
    P, seed = 4096, 1
    m = _pin_model(nominal=NOMINAL if variant == "nominal" else None, process_var=np.array([0.004, 0.002]) if variant == "process_var" else None)
    pb = _pin_problem()
    X, S2 = R.rollout(m, pb["x0"][None], pb["u0"][None, None], P, seed=seed)
    assert S2.min() > 0.0, "a clamped particle"
    x1 = X[1, 0]
    mu, var = _oracle_moments(m, np.concatenate((pb["x0"], pb["u0"])), np.diag([0.05, 0.02, 0.01]))
    mean_mc, d = x1.mean(axis=0), x1 - x1.mean(axis=0)
    var_mc = (d ** 2).sum(axis=0) / (P - 1)
    m4 = (d ** 4).mean(axis=0)
    z_mean = (mean_mc - mu) / np.sqrt(var_mc / P)
    z_var = (var_mc - var) / np.sqrt((m4 - var_mc ** 2) / P)
    print("  %s: min s2 %.2e; z(mean) %s, z(var) %s" % (variant, S2.min(), np.round(z_mean, 2), np.round(z_var, 2)))
    assert np.all(np.abs(z_mean) <= 4.0) and np.all(np.abs(z_var) <= 4.0)
    # ... and the initial draw has the requested covariance (same rule)
    d0 = X[0, 0] - X[0, 0].mean(axis=0)
    v0 = (d0 ** 2).sum(axis=0) / (P - 1)
    z0 = (v0 - np.array([0.05, 0.02])) / np.sqrt(((d0 ** 4).mean(axis=0) - v0 ** 2) / P)
    assert np.all(np.abs(z0) <= 4.0) and np.all(np.abs(X[0, 0].mean(axis=0) - pb["x0"]) <= 4.0 * np.sqrt(v0 / P))


def test_noise_addressing():
    """A value depends on (seed, call_index, p, t, element) only: not on P, not on the number of normals asked for; other streams differ."""
    a, b = R.normals(7, 3, 2, 16, 3), R.normals(7, 3, 2, 5, 3)
    assert np.array_equal(a[:5], b)
    assert np.array_equal(R.normals(7, 3, 2, 16, 5)[:, :3], a[:, :3][:, :3]) and np.array_equal(R.normals(7, 3, 2, 16, 4)[:, :3], a)
    for other in (R.normals(8, 3, 2, 16, 3), R.normals(7, 4, 2, 16, 3), R.normals(7, 3, 1, 16, 3), R.normals(7 + (1 << 32), 3, 2, 16, 3)):
        assert not np.any(other == a)
    import mppi_reference as MR
    assert not np.any(np.isin(MR.normals(7, 3, 2, 48), a))                 # the key keeps the particle streams apart from MPPI's
    # plans share draws (common random numbers), B does not matter: plan b of a batch of 3 is the plan alone
    m = _pin_model()
    x0 = np.array([[0.3, -0.2], [0.1, 0.4], [-0.5, 0.0]])
    U = np.array([[[0.4], [0.1]], [[-0.2], [0.3]], [[0.0], [0.0]]])
    X3, _ = R.rollout(m, x0, U, 9, seed=5)
    X1, _ = R.rollout(m, x0[1:2], U[1:2], 9, seed=5)
    X1s, _ = R.rollout(m, x0[1:2], U[1:2], 4, seed=5)
    assert np.array_equal(X3[:, 1], X1[:, 0]) and np.array_equal(X1[:, 0, :4], X1s[:, 0])
    assert np.array_equal(X3[0, 0] - x0[0], X3[0, 1] - x0[1]) or np.allclose(X3[0, 0] - x0[0], X3[0, 1] - x0[1], rtol=0, atol=1e-15)


def test_zero_pivot_in_init_cov():
    """Zero variances are legal: a zero pivot gives a zero column of the factor, and L L^T is still the matrix."""
    for P in (np.diag([0.04, 0.0]), np.diag([0.0, 0.0]), np.full((2, 2), 0.25), np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.5], [0.0, 0.5, 0.25]])):
        Lc = R.cholesky_lower(P)
        assert np.all(np.isfinite(Lc)) and np.allclose(Lc @ Lc.T, P, rtol=0, atol=1e-15) and np.array_equal(Lc, np.tril(Lc))
    assert np.array_equal(R.cholesky_lower(np.full((2, 2), 0.25)), np.array([[0.5, 0.0], [0.5, 0.0]]))
    with pytest.raises(ValueError):
        R.cholesky_lower(np.array([[1.0, 2.0], [2.0, 1.0]]))
    m = dict(_pin_model(), init_cov=np.diag([0.04, 0.0]))
    X0 = R.initial(m, np.array([[0.3, -0.2]]), 8, 3, 0)
    assert np.all(X0[0, :, 1] == -0.2) and np.std(X0[0, :, 0]) > 0
