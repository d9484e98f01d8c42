"""Extended-precision restatement of the linearised propagation (gpmpc_linearised_step, gpmpc_linearised_rollout; include/gpmpc.h,
"Linearised propagation").  TEST INFRASTRUCTURE ONLY.

Conventions of tests/particle_reference.py and tests/gpstate_reference.py: ``np.longdouble`` where the host has it, the float64 Kinv is data,
a model is the dict of particle_reference, the definitions are written out with none of the kernels' groupings (no tiles, no chunks, no GP
groups), and every sum comes back with the sum of the absolute values of its terms, which is what the GPU tests bound by ``tol * sum |terms|``.

One step at z = (mu, u), S = (var, action_var), d_id = (X_id - z_d) / lambda_d:
    m = sum_i beta_i k_i [+ W . z + b]         g_d = sum_i beta_i k_i d_id [+ W_d]       q = sum_ij k_i K_ij k_j
    r = (K + K^T) k       dq_d = sum_i r_i k_i d_id       w = g o S       h_d = sum_i beta_i k_i (d_id (d_i . w) - w_d / lambda_d)
    mu' = m               var' = (sf^2 - q) + sum_d g_d^2 S_d + process_var
    Jacobian [2ds][2ds+da], rows (mu', var'), columns (mu, var, u):  row mu': g | 0 | g;   row var': -dq + 2h | g_k^2 | -dq + 2h

Budgets of the composite outputs, in units of ``sum |terms|`` (so that a bound is tol * budget [+ a few ulp of ``mag``, the sizes that the
last float64 additions round at]), carried through the formulas:
    var'            q_abs + sum_d 2 |g_d| S_d g_abs_d
    J[var'][mu, u]  dq_abs + 2 (h_abs + sum_l Habs_dl S_l g_abs_l),  Habs_dl = sum_i |beta_i k_i| |d_id d_il - [d = l] / lambda_d|: h is linear
                    in w = g o S, and the g the device multiplies by S carries its own budget
    J[var'][var_k]  2 |g_k| g_abs_k

Keyword switches for deliberate MISTAKES (the discriminating controls):
    r_twice          r = 2 K k instead of (K + K^T) k   (shows only on a Kinv that is visibly not symmetric)
    drop_h           the h term left out of the variance rows
    drop_nominal_g   the nominal weights W left out of g (and with it of var' and the Jacobian)
"""
import numpy as np

import cost_reference as C
import gpstate_reference as G
import particle_reference as P

dims, noise_model = P.dims, P.noise_model


def make_model(n, ds, da, kind="pergp", seed=0, sn=0.1, noise=False, nominal=False, pair=False, groups=None):
    """A GP bundle on random inputs (the generator of tests/test_gpu_particles.py).  kind: pergp (per-GP hyper-parameters and inverses) |
    shared (one hyper-parameter set, ONE inverse: gp_stride = 0) | nonsym (per-GP, every entry of the inverse perturbed by a relative 1e-3:
    visibly not symmetric).  pair: the GPs 0 and 2 share (lambda, sigma_f), GP 1 stands apart (two groups, the first with a gap).
    groups: a list of index lists, each sharing the (lambda, sigma_f) of its first member; pair is groups=[[0, 2]].  Nothing is drawn for
    it: with groups=None every array is what it was before the argument existed.
    noise: a non-default init_cov diagonal, action_var and process_var."""
    rng = np.random.default_rng(100 * n + 10 * ds + da + seed)
    D = ds + da
    X = rng.uniform(-1.5, 1.5, (n, D))
    lam = rng.uniform(1.0, 3.0, (ds, D))
    sf = rng.uniform(0.6, 1.8, ds)
    if kind == "shared":
        lam, sf = np.tile(lam[:1], (ds, 1)), np.tile(sf[:1], ds)
    else:
        for members in ([[0, 2]] if pair else []) + [list(g) for g in (groups or [])]:
            for a in members[1:]:
                lam[a], sf[a] = lam[members[0]], sf[members[0]]
    Y = np.stack([np.sin(X @ rng.standard_normal(D)) for _ in range(ds)], axis=1) + sn * rng.standard_normal((n, ds))
    Ks = []
    for a in range(ds):
        K = G.to_f64(G.kernel(X, X, lam[a], sf[a])) + sn * sn * np.eye(n)
        Ki = np.linalg.inv(K)                                             # LU: not symmetric to the last bit
        if kind == "nonsym":
            Ki = Ki * (1.0 + 1e-3 * rng.standard_normal((n, n)))
        Ks.append(Ki)
    Kinv = Ks[0] if kind == "shared" else np.stack(Ks)
    beta = np.stack([Ks[a] @ Y[:, a] for a in range(ds)], axis=1)
    m = dict(X=X, beta=beta, Kinv=Kinv, lam=lam, sf=sf, kind=kind)
    if noise:
        m.update(init_cov=np.diag(rng.uniform(1e-3, 4e-3, ds)), action_var=rng.uniform(5e-4, 3e-3, da), process_var=rng.uniform(1e-3, 4e-3, ds))
    if nominal:
        m["nominal"] = (0.3 * rng.standard_normal((ds, D)), 0.05 * rng.standard_normal(ds))
    return m


def make_inputs(model, B, seed=3):
    """mu (B, ds) in the data's range, var (B, ds) in [1e-3, 5e-2], U_t (B, da)."""
    ds, da, _ = dims(model)
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.2, 1.2, (B, ds)), rng.uniform(1e-3, 5e-2, (B, ds)), rng.uniform(-1.2, 1.2, (B, da))


def _inputs(model, mu, var, U_t):
    ds, da, D = dims(model)
    mu = np.asarray(mu, dtype=np.float64).reshape(-1, ds)
    B = mu.shape[0]
    var = np.asarray(var, dtype=np.float64).reshape(B, ds)
    U_t = np.zeros((B, 0)) if da == 0 else np.asarray(U_t, dtype=np.float64).reshape(B, da)
    return mu, var, U_t


def step(model, mu, var, U_t, prec=None, r_twice=False, drop_h=False, drop_nominal_g=False):
    """mu, var (B, ds), U_t (B, da) -> dict in the working precision:
    m, m_abs, q, q_abs, mu, var, var_abs, var_mag (B, ds); g, g_abs, dq, dq_abs, h, h_abs (B, ds, D); jac, jac_abs, jac_mag (B, 2ds, 2ds+da)."""
    ds, da, D = dims(model)
    mu, var, U_t = (G.cast(a, prec) for a in _inputs(model, mu, var, U_t))
    B = mu.shape[0]
    _, av, pv = noise_model(model)
    Z = np.concatenate([mu, U_t], axis=1)
    S = np.concatenate([var, np.broadcast_to(G.cast(av, prec), (B, da))], axis=1)
    X = G.cast(model["X"], prec)
    beta = G.cast(model["beta"], prec)
    nominal = model.get("nominal")
    nz, nc = 2 * ds, 2 * ds + da
    col = [d if d < ds else ds + d for d in range(D)]
    keys = ("m", "m_abs", "q", "q_abs", "mu", "var", "var_abs", "var_mag", "g", "g_abs", "dq", "dq_abs", "h", "h_abs")
    cols = {k: [] for k in keys}
    jac = np.zeros((B, nz, nc), dtype=Z.dtype)
    jac_abs, jac_mag = jac.copy(), jac.copy()
    for a in range(ds):
        lam, sf = G.cast(model["lam"][a], prec), G.cast(model["sf"][a], prec)
        n = X.shape[0]
        e = np.zeros((n, B), dtype=Z.dtype)
        for k in range(D):
            dk = X[:, k][:, None] - Z[:, k][None, :]
            e = e + dk * dk / lam[k]
        ks = sf * sf * G._exp(-e / 2)                                              # (n, B)
        d = (X[:, None, :] - Z[None, :, :]) / lam[None, None, :]                   # (n, B, D)
        bk = beta[:, a][:, None] * ks
        abk, ad, aks = G._abs(bk), G._abs(d), G._abs(ks)
        m, m_abs = bk.sum(axis=0), abk.sum(axis=0)
        gt = bk[:, :, None] * d
        g, g_abs = gt.sum(axis=0), G._abs(gt).sum(axis=0)
        if nominal is not None:
            W = G.cast(np.asarray(nominal[0], dtype=np.float64)[a], prec)
            b = G.cast(np.broadcast_to(np.asarray(nominal[1], dtype=np.float64), (ds,))[a], prec)
            m, m_abs = m + Z @ W + b, m_abs + G._abs(Z) @ G._abs(W) + abs(b)       # (the nominal terms are terms of the sum too)
            if not drop_nominal_g:
                g, g_abs = g + W[None, :], g_abs + G._abs(W)[None, :]
        K = G.cast(P._kinv(model, a), prec)
        aK = G._abs(K)
        q = (ks * (K @ ks)).sum(axis=0)                                            # sum_i sum_j k_i K_ij k_j: ALL entries
        q_abs = (aks * (aK @ aks)).sum(axis=0)
        r = (K + K) @ ks if r_twice else (K + K.T) @ ks
        r_abs = (aK + aK.T) @ aks
        dq = ((r * ks)[:, :, None] * d).sum(axis=0)
        dq_abs = ((r_abs * aks)[:, :, None] * ad).sum(axis=0)
        w = g * S
        aw = G._abs(w)
        dw = (d * w[None, :, :]).sum(axis=2)
        adw = (ad * aw[None, :, :]).sum(axis=2)
        ht = bk[:, :, None] * (d * dw[:, :, None] - (w / lam[None, :])[None, :, :])
        h = ht.sum(axis=0)
        h_abs = (abk[:, :, None] * (ad * adw[:, :, None] + (aw / lam[None, :])[None, :, :])).sum(axis=0)
        # |second derivative| entry by entry, for the budget h inherits from the g inside w
        Habs = np.einsum("ib,ibd,ibl->bdl", abk, ad, ad)
        for k in range(D):
            Habs[:, k, k] = Habs[:, k, k] + abk.sum(axis=0) / lam[k]
        h_abs = h_abs + np.einsum("bdl,bl->bd", Habs, S * g_abs)
        if drop_h:
            h = h * 0
        lin = (g * g * S).sum(axis=1)
        var_n = (sf * sf - q) + lin + G.cast(pv[a], prec)
        var_abs = q_abs + (2 * G._abs(g) * S * g_abs).sum(axis=1)
        var_mag = sf * sf + G._abs(q) + G._abs(lin) + G.cast(pv[a], prec)
        for k, v in zip(keys, (m, m_abs, q, q_abs, m, var_n, var_abs, var_mag, g, g_abs, dq, dq_abs, h, h_abs)):
            cols[k].append(v)
        for k in range(D):
            jac[:, a, col[k]], jac_abs[:, a, col[k]], jac_mag[:, a, col[k]] = g[:, k], g_abs[:, k], G._abs(g[:, k])
            jac[:, ds + a, col[k]] = -dq[:, k] + 2 * h[:, k]
            jac_abs[:, ds + a, col[k]] = dq_abs[:, k] + 2 * h_abs[:, k]
            jac_mag[:, ds + a, col[k]] = G._abs(dq[:, k]) + 2 * G._abs(h[:, k])
            if k < ds:
                jac[:, ds + a, ds + k] = g[:, k] * g[:, k]
                jac_abs[:, ds + a, ds + k] = 2 * G._abs(g[:, k]) * g_abs[:, k]
                jac_mag[:, ds + a, ds + k] = g[:, k] * g[:, k]
    out = {k: np.stack(v, axis=1) for k, v in cols.items()}
    out.update(jac=jac, jac_abs=jac_abs, jac_mag=jac_mag)
    return out


def rollout(model, x0, U, prec=None, **mistakes):
    """The chain of steps in the working precision, nothing rounded in between: means, vars (B, H+1, ds), jac (B, H, 2ds, 2ds+da)."""
    ds, da, D = dims(model)
    U = np.asarray(U, dtype=np.float64)
    B, H = U.shape[0], U.shape[1]
    x0 = np.broadcast_to(np.asarray(x0, dtype=np.float64).reshape(-1, ds), (B, ds))
    P0, _, _ = noise_model(model)
    means, vars_ = [G.cast(x0, prec)], [G.cast(np.broadcast_to(np.diag(P0), (B, ds)), prec)]
    jac = []
    for t in range(H):
        r = step(model, means[-1], vars_[-1], U[:, t], prec, **mistakes)
        means.append(r["mu"])
        vars_.append(r["var"])
        jac.append(r["jac"])
    return {"means": np.stack(means, axis=1), "vars": np.stack(vars_, axis=1), "jac": np.stack(jac, axis=1)}


def adjoint(jac, means, vars_, U, gamma, Q, R, **cost_kw):
    """Cost and gradient of given trajectories, the arithmetic that follows the steps: the risk-sensitive cost on the DIAGONAL covariances
    and the reverse sweep over the step Jacobians (tests/cost_reference.py).  Returns dict(cost, A_cost (B,), grad, A_grad (B, H, da)):
    A_* are the error units (sums of the absolute terms, carried through the sweep over |J|)."""
    means, vars_ = np.asarray(means), np.asarray(vars_)
    B, H1, ds = means.shape
    covs = np.zeros((B, H1, ds, ds), dtype=vars_.dtype)
    for k in range(ds):
        covs[..., k, k] = vars_[..., k]
    t = C.cost_terms(means, covs, U, gamma, Q, R, **cost_kw)
    gU, _ = C.sweep(jac, t["dmu"], t["dvar"])
    aU, _ = C.sweep_unit(jac, t["A_dmu"], t["A_dvar"])
    return {"cost": t["value"], "A_cost": t["A_value"], "grad": t["dU"] + gU, "A_grad": t["A_dU"] + aU}


def cost_gradient(model, x0, U, gamma, Q, R, prec=None, mistakes=None, **cost_kw):
    """The adjoint (cost gradient) of a rollout, all of it in the working precision: rollout() then adjoint()."""
    r = rollout(model, x0, U, prec, **(mistakes or {}))
    r.update(adjoint(r["jac"], r["means"], r["vars"], U, gamma, Q, R, **cost_kw))
    return r
