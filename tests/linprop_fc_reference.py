"""Extended-precision restatement of the full-covariance linearised propagation with a linear state feedback (gpmpc_linearised_fc_step,
gpmpc_linearised_fc_rollout, gpmpc_linearised_fc_vjp, gpmpc_linearised_fc_constraints; include/gpmpc.h, "Linearised propagation, full
covariance").  TEST INFRASTRUCTURE ONLY.

Built on tests/linprop_reference.py (whose ``step`` supplies m, g, q, dq/dz and their term sums: none of them depends on the input
covariance) and tests/particle_reference.py (the model dict, the noise model, the inverse of GP a).  Conventions as there: ``np.longdouble``,
the float64 Kinv and gain are data, the rule is written out with none of the kernels' groupings (no tiles, no chunks, no stage A / close
split), and every sum comes back with the sum of the absolute values of its terms.

One step at zbar = (mu, v) under u = v + K (x - mu), D = ds + da, T = [I; K]:
    Hm_a[d][l] = sum_i beta_ia k_i (d_id d_il - [d = l] / lambda_ad)
    Sz  = T Sigma T^T + diag(0, action_var)        P_a = G_a T        W_b = Sz G_b^T
    mu'_a = m_a        Sigma'_ab = [a = b] (sf_a^2 - q_a + process_var_a) + G_a . W_b
    packed state s = (mu, Sigma_kl for k <= l row-major), p = ds + ds (ds + 1) / 2; Jacobian [p][p + da], rows s', columns (s, v):
    d mu'_a / d mu_k = g_ak,  / d v_j = g_a,ds+j,  / d Sigma_kl = 0
    d Sigma'_ab / d zbar_d = -[a = b] dq_a/dz_d + (Hm_a W_b)_d + (Hm_b W_a)_d
    d Sigma'_ab / d Sigma_kl = P_ak P_bl + P_al P_bk (k < l),  P_ak P_bk (k = l)

Budgets, in units of ``sum |terms|`` (a bound is TOL * budget + 4 ulp of ``mag``, the size at which the last float64 additions round).  The
inputs Sigma, K, action_var are data; g, q, dq come with the budgets g_abs, q_abs, dq_abs of linprop_reference; |x| is entry by entry:
    Sz_abs       = |T| |Sigma| |T|^T + diag(0, action_var)                       (every grouping of the triple product has these terms)
    W_abs_b[d]   = sum_l ( Sz_abs[d][l] |G_b[l]| + |Sz[d][l]| g_abs_b[l] )        (the sum's own terms, and the g it inherits)
    Sigma'_ab    : [a = b] q_abs_a + sum_d ( g_abs_a[d] |W_b[d]| + |G_a[d]| W_abs_b[d] );   mag = [a = b] (sf^2 + |q| + pv) + |G_a . W_b|
    P_abs_a[k]   = g_abs_a[k] + sum_j g_abs_a[ds+j] |K_jk|                        (g_abs >= |g|: the terms of the sum are covered)
    J[Sigma'_ab][Sigma_kl] : sum over the one or two products of  P_abs |P| + |P| P_abs;   mag = the sum of the |products|
    Habs_a[d][l] = sum_i |beta_i k_i| (|d_id d_il| + [d = l] / lambda_d)
    (Hm_a W_b)_d : HW_abs = sum_l ( Habs_a[d][l] |W_b[l]| + |Hm_a[d][l]| W_abs_b[l] )
    J[Sigma'_ab][zbar_d]   : [a = b] dq_abs_a[d] + HW_abs(a, b) + HW_abs(b, a);   mag = [a = b] |dq| + |Hm_a W_b| + |Hm_b W_a|
    J[mu'_a][.]  : g_abs;  mag = |g|
Entries whose budget is zero are structural zeros (d mu' / d Sigma) and are asserted as exact zeros.

Keyword switches for deliberate MISTAKES (the discriminating controls):
    drop_cross_hess          Hm_b W_a left out of the zbar columns
    feedback_cross_dropped   a block-diagonal Sz: K Sigma K^T + action_var in the input block, but no Sigma K^T beside it
    offdiag_once             d / d Sigma_kl counted once for k < l: P_ak P_bl only
"""
import numpy as np

import cost_reference as C
import gpstate_reference as G
import linprop_reference as R
import particle_reference as P

dims, noise_model, make_model = R.dims, R.noise_model, R.make_model
_abs = G._abs


def packed_dim(ds):
    return ds + ds * (ds + 1) // 2


def tri_pairs(n):
    """The (k, l), k <= l, of the row-major upper triangle."""
    return [(k, l) for k in range(n) for l in range(k, n)]


def make_inputs(model, B, seed=3, gain=True):
    """mu (B, ds) in the data's range, a non-diagonal SPD cov (B, ds, ds), U_t (B, da), a gain (da, ds) of entries in [-0.5, 0.5]."""
    ds, da, _ = dims(model)
    rng = np.random.default_rng(seed)
    mu, U = rng.uniform(-1.2, 1.2, (B, ds)), rng.uniform(-1.2, 1.2, (B, da))
    A = rng.standard_normal((B, ds, ds))
    cov = 0.02 * np.einsum("bij,bkj->bik", A, A) / ds + 2e-3 * np.eye(ds)
    cov = 0.5 * (cov + np.swapaxes(cov, 1, 2))
    K = rng.uniform(-0.5, 0.5, (da, ds)) if gain and da else None
    return mu, cov, U, K


def _hessians(model, Z, prec):
    """Hm, Habs (B, ds, D, D): the second derivative of each GP's mean at the columns Z (B, D), and its absolute term sums."""
    ds, da, D = dims(model)
    X, beta = G.cast(model["X"], prec), G.cast(model["beta"], prec)
    B = Z.shape[0]
    Hm = np.zeros((B, ds, D, D), dtype=Z.dtype)
    Ha = Hm.copy()
    for a in range(ds):
        lam, sf = G.cast(model["lam"][a], prec), G.cast(model["sf"][a], prec)
        e = np.zeros((X.shape[0], B), dtype=Z.dtype)
        for k in range(D):
            dk = X[:, k][:, None] - Z[:, k][None, :]
            e = e + dk * dk / lam[k]
        ks = sf * sf * G._exp(-e / 2)
        d = (X[:, None, :] - Z[None, :, :]) / lam[None, None, :]
        bk = beta[:, a][:, None] * ks
        abk, ad = _abs(bk), _abs(d)
        for k in range(D):
            for l in range(D):
                Hm[:, a, k, l] = (bk * d[:, :, k] * d[:, :, l]).sum(axis=0)
                Ha[:, a, k, l] = (abk * ad[:, :, k] * ad[:, :, l]).sum(axis=0)
            Hm[:, a, k, k] = Hm[:, a, k, k] - bk.sum(axis=0) / lam[k]
            Ha[:, a, k, k] = Ha[:, a, k, k] + abk.sum(axis=0) / lam[k]
    return Hm, Ha


def step(model, mu, cov, U_t, K=None, prec=None, drop_cross_hess=False, feedback_cross_dropped=False, offdiag_once=False):
    """mu (B, ds), cov (B, ds, ds) (the upper triangle is read), U_t (B, da), K (da, ds) or None -> dict in the working precision:
    mu, m_abs (B, ds); cov, cov_abs, cov_mag (B, ds, ds); jac, jac_abs, jac_mag (B, p, p + da); G, P, W, Sz, Hm."""
    ds, da, D = dims(model)
    mu = np.asarray(mu, dtype=np.float64).reshape(-1, ds)
    B = mu.shape[0]
    cov = np.asarray(cov, dtype=np.float64).reshape(B, ds, ds)
    cov = np.triu(cov) + np.swapaxes(np.triu(cov, 1), 1, 2)
    U_t = np.zeros((B, 0)) if da == 0 else np.asarray(U_t, dtype=np.float64).reshape(B, da)
    base = R.step(model, mu, np.zeros((B, ds)), U_t, prec)
    dt = base["m"].dtype
    _, av, pv = noise_model(model)
    av, pv = G.cast(np.asarray(av, dtype=np.float64), prec), G.cast(np.asarray(pv, dtype=np.float64), prec)
    Sg = G.cast(cov, prec)
    Kg = np.zeros((da, ds), dtype=dt) if K is None else G.cast(np.asarray(K, dtype=np.float64).reshape(da, ds), prec)
    T = np.concatenate([np.eye(ds, dtype=dt), Kg], axis=0)                            # (D, ds)
    Sz = np.einsum("dk,bkl,el->bde", T, Sg, T)
    Sz_abs = np.einsum("dk,bkl,el->bde", _abs(T), _abs(Sg), _abs(T))
    if feedback_cross_dropped:
        Sz[:, :ds, ds:] = 0
        Sz[:, ds:, :ds] = 0
    for j in range(da):
        Sz[:, ds + j, ds + j] = Sz[:, ds + j, ds + j] + av[j]
        Sz_abs[:, ds + j, ds + j] = Sz_abs[:, ds + j, ds + j] + av[j]
    g, g_abs = base["g"], base["g_abs"]                                              # (B, ds, D)
    W = np.einsum("bdl,bal->bad", Sz, g)                                             # W[b][a][d] = sum_l Sz[d][l] G_a[l]
    W_abs = np.einsum("bdl,bal->bad", Sz_abs, _abs(g)) + np.einsum("bdl,bal->bad", _abs(Sz), g_abs)
    # (da = 0: no sum at all -- numpy's einsum over an EMPTY axis of a long double slice hands back memory it never wrote)
    Pm = g[:, :, :ds] + (np.einsum("baj,jk->bak", g[:, :, ds:], Kg) if da else 0)
    P_abs = g_abs[:, :, :ds] + (np.einsum("baj,jk->bak", g_abs[:, :, ds:], _abs(Kg)) if da else 0)
    s2 = (G.cast(np.asarray(model["sf"], dtype=np.float64), prec) ** 2)[None, :] - base["q"] + pv[None, :]
    s2_mag = (G.cast(np.asarray(model["sf"], dtype=np.float64), prec) ** 2)[None, :] + _abs(base["q"]) + pv[None, :]
    GW = np.einsum("bad,bcd->bac", g, W)                                             # G_a . W_c
    cov_n = GW.copy()
    cov_abs = np.einsum("bad,bcd->bac", g_abs, _abs(W)) + np.einsum("bad,bcd->bac", _abs(g), W_abs)
    cov_mag = _abs(GW)
    for a in range(ds):
        cov_n[:, a, a] = s2[:, a] + GW[:, a, a]
        cov_abs[:, a, a] = cov_abs[:, a, a] + base["q_abs"][:, a]
        cov_mag[:, a, a] = cov_mag[:, a, a] + s2_mag[:, a]
    Z = G.cast(np.concatenate([mu, U_t], axis=1), prec)
    Hm, Ha = _hessians(model, Z, prec)
    HW = np.einsum("badl,bcl->bacd", Hm, W)                                          # HW[b][a][c][d] = (Hm_a W_c)_d
    HW_abs = np.einsum("badl,bcl->bacd", Ha, _abs(W)) + np.einsum("badl,bcl->bacd", _abs(Hm), W_abs)
    pairs = tri_pairs(ds)
    p = packed_dim(ds)
    nc = p + da
    zcol = [d if d < ds else p + (d - ds) for d in range(D)]
    jac = np.zeros((B, p, nc), dtype=dt)
    jac_abs, jac_mag = jac.copy(), jac.copy()
    for a in range(ds):
        for d in range(D):
            jac[:, a, zcol[d]], jac_abs[:, a, zcol[d]], jac_mag[:, a, zcol[d]] = g[:, a, d], g_abs[:, a, d], _abs(g[:, a, d])
    for r, (a, b) in enumerate(pairs):
        row = ds + r
        for d in range(D):
            v = HW[:, a, b, d] + (0 if drop_cross_hess else HW[:, b, a, d])
            va = HW_abs[:, a, b, d] + HW_abs[:, b, a, d]
            vm = _abs(HW[:, a, b, d]) + _abs(HW[:, b, a, d])
            if a == b:
                v, va, vm = v - base["dq"][:, a, d], va + base["dq_abs"][:, a, d], vm + _abs(base["dq"][:, a, d])
            jac[:, row, zcol[d]], jac_abs[:, row, zcol[d]], jac_mag[:, row, zcol[d]] = v, va, vm
        for c, (k, l) in enumerate(pairs):
            t1 = Pm[:, a, k] * Pm[:, b, l]
            a1 = P_abs[:, a, k] * _abs(Pm[:, b, l]) + _abs(Pm[:, a, k]) * P_abs[:, b, l]
            if k == l:
                v, va, vm = t1, a1, _abs(t1)
            else:
                t2 = Pm[:, a, l] * Pm[:, b, k]
                a2 = P_abs[:, a, l] * _abs(Pm[:, b, k]) + _abs(Pm[:, a, l]) * P_abs[:, b, k]
                v, va, vm = (t1 if offdiag_once else t1 + t2), a1 + a2, _abs(t1) + _abs(t2)
            jac[:, row, ds + c], jac_abs[:, row, ds + c], jac_mag[:, row, ds + c] = v, va, vm
    return {"mu": base["m"], "m_abs": base["m_abs"], "cov": cov_n, "cov_abs": cov_abs, "cov_mag": cov_mag, "jac": jac, "jac_abs": jac_abs,
            "jac_mag": jac_mag, "G": g, "P": Pm, "W": W, "Sz": Sz, "Hm": Hm, "base": base}


def pack_state(mu, cov):
    """(B, ds), (B, ds, ds) -> (B, p)"""
    ds = mu.shape[-1]
    return np.concatenate([mu] + [cov[..., k, l][..., None] for k, l in tri_pairs(ds)], axis=-1)


def pack_cov_seed(g):
    """Upstream gradients of a full matrix (..., ds, ds) -> those of the packed variables (..., nt): g_kl + g_lk for k < l."""
    ds = g.shape[-1]
    return np.stack([g[..., k, k] if k == l else g[..., k, l] + g[..., l, k] for k, l in tri_pairs(ds)], axis=-1)


def gain_at(K, t, ds, da):
    """The gain of step t (0-based) from None, (da, ds) or (H, da, ds)."""
    if K is None:
        return None
    K = np.asarray(K, dtype=np.float64)
    return K if K.ndim == 2 else K[t]


def chain(model, x0, U, K=None, prec=None, **mistakes):
    """The chain of steps: means (B, H+1, ds), covs (B, H+1, ds, ds), jac (B, H, p, p+da) in the working precision, and the steps' own dicts.
    A step takes float64 inputs, as linprop_reference.step does: the state is rounded to float64 between steps, each step is exact to the
    working precision from there.  K: None, (da, ds) or (H, da, ds)."""
    ds, da, D = dims(model)
    U = np.asarray(U, dtype=np.float64)
    B, H = U.shape[0], U.shape[1]
    x0 = np.broadcast_to(np.asarray(x0, dtype=np.float64).reshape(-1, ds), (B, ds))
    P0, _, _ = noise_model(model)
    means, covs, jac, steps = [G.cast(x0, prec)], [G.cast(np.broadcast_to(np.asarray(P0, dtype=np.float64), (B, ds, ds)), prec)], [], []
    for t in range(H):
        r = step(model, G.to_f64(means[-1]), G.to_f64(covs[-1]), U[:, t], gain_at(K, t, ds, da), prec, **mistakes)
        means.append(r["mu"])
        covs.append(r["cov"])
        jac.append(r["jac"])
        steps.append(r)
    return {"means": np.stack(means, axis=1), "covs": np.stack(covs, axis=1), "jac": np.stack(jac, axis=1), "steps": steps}


def sweep(J, g_means=None, g_covs=None, dtype=G.LD):
    """Reverse sweep over packed Jacobians J (B, H, p, p + da) with seeds g_means (B, H+1, ds), g_covs (B, H+1, ds, ds) at every step:
    gU (B, H, da), gx0 (B, ds).  The adjoint of Sigma_kl, k < l, is g_covs[k][l] + g_covs[l][k]."""
    J = np.asarray(J, dtype=dtype)
    B, H, p, nc = J.shape
    ds = next(d for d in range(1, 64) if packed_dim(d) == p)

    def seed(t):
        a = np.zeros((B, p), dtype=dtype)
        if g_means is not None:
            a[:, :ds] = np.asarray(g_means, dtype=dtype)[:, t]
        if g_covs is not None:
            a[:, ds:] = pack_cov_seed(np.asarray(g_covs, dtype=dtype)[:, t])
        return a
    adj = seed(H)
    gU = np.zeros((B, H, nc - p), dtype=dtype)
    for t in range(H, 0, -1):
        s = np.einsum("brc,br->bc", J[:, t - 1], adj)
        gU[:, t - 1] = s[:, p:]
        adj = seed(t - 1) + s[:, :p]
    return gU, adj[:, :ds]


def adjoint(jac, means, covs, U, gamma, Q, Rm, **cost_kw):
    """Cost and gradient of given trajectories: the risk-sensitive cost on the FULL covariances (tests/cost_reference.py) and the reverse
    sweep over the packed Jacobians.  dict(cost, A_cost (B,), grad, A_grad (B, H, da)); A_*: the error units, carried through |J|."""
    t = C.cost_terms(np.asarray(means), np.asarray(covs), U, gamma, Q, Rm, **cost_kw)
    gU, _ = sweep(jac, t["dmu"], t["dsig"])
    aU, _ = sweep(np.abs(np.asarray(jac, dtype=G.LD)), np.abs(t["A_dmu"]), np.abs(t["A_dsig"]))
    return {"cost": t["value"], "A_cost": t["A_value"], "grad": t["dU"] + gU, "A_grad": t["A_dU"] + aU, "dmu": t["dmu"], "dsig": t["dsig"]}


def constraints(means, covs, jac, A, b, kappa, dtype=G.LD):
    """g (B, H, m) = a . mu_t + kappa sqrt(a^T Sigma_t a) - b and the dense Jacobian (B, H m, H da) by the forward-sensitivity sweep over the
    packed Jacobians, with the error units A_g, A_gjac (sums of absolute terms; S carried through |J|).  A radicand <= 0: sd = 0 and no
    variance part.  jac None: values only."""
    means, covs = np.asarray(means, dtype=dtype), np.asarray(covs, dtype=dtype)
    A, b, kappa = np.asarray(A, dtype=dtype), np.asarray(b, dtype=dtype), np.asarray(kappa, dtype=dtype)
    B, H1, ds = means.shape
    H, m = H1 - 1, A.shape[0]
    am = np.einsum("rk,btk->btr", A, means[:, 1:])
    am_abs = np.einsum("rk,btk->btr", np.abs(A), np.abs(means[:, 1:]))
    q = np.einsum("rk,btkl,rl->btr", A, covs[:, 1:], A)
    q_abs = np.einsum("rk,btkl,rl->btr", np.abs(A), np.abs(covs[:, 1:]), np.abs(A))
    pos = q > 0
    sd = np.where(pos, np.sqrt(np.where(pos, q, 1)), 0)
    out = {"g": am + kappa[None, None, :] * sd - b[None, None, :], "sd": sd, "q": q,
           "A_g": am_abs + np.abs(b)[None, None, :] + kappa[None, None, :] * (sd + np.where(pos, q_abs / (2 * np.where(pos, sd, 1)), 0))}
    if jac is None:
        return out
    J = np.asarray(jac, dtype=dtype)
    p, nc = J.shape[2], J.shape[3]
    da = nc - p
    pairs = tri_pairs(ds)
    wts = np.stack([A[:, k] * A[:, l] * (1 if k == l else 2) for k, l in pairs], axis=1)             # (m, nt)
    f = np.where(pos, kappa[None, None, :] / (2 * np.where(pos, sd, 1)), 0)
    S, Sa = np.zeros((B, p, H * da), dtype=dtype), np.zeros((B, p, H * da), dtype=dtype)
    gj, gja = np.zeros((B, H * m, H * da), dtype=dtype), np.zeros((B, H * m, H * da), dtype=dtype)
    for t in range(1, H + 1):
        Jt = J[:, t - 1]
        S, Sa = np.einsum("brk,bkc->brc", Jt[:, :, :p], S), np.einsum("brk,bkc->brc", np.abs(Jt[:, :, :p]), Sa)
        S[:, :, (t - 1) * da:t * da] = Jt[:, :, p:]
        Sa[:, :, (t - 1) * da:t * da] = np.abs(Jt[:, :, p:])
        S[:, :, t * da:] = 0
        Sa[:, :, t * da:] = 0
        dm, dv = np.einsum("rk,bkc->brc", A, S[:, :ds]), np.einsum("rv,bvc->brc", wts, S[:, ds:])
        dma, dva = np.einsum("rk,bkc->brc", np.abs(A), Sa[:, :ds]), np.einsum("rv,bvc->brc", np.abs(wts), Sa[:, ds:])
        ft = f[:, t - 1, :, None]
        rel = np.where(pos[:, t - 1], q_abs[:, t - 1] / np.where(pos[:, t - 1], q[:, t - 1], 1), 0)[:, :, None]
        gj[:, (t - 1) * m:t * m] = dm + ft * dv
        gja[:, (t - 1) * m:t * m] = dma + np.abs(ft) * dva + np.abs(ft * dv) * (1 + rel)
    out.update(gjac=gj, A_gjac=gja)
    return out
