"""Extended-precision restatement of the particle entry points (gpmpc_gp_posterior, gpmpc_particle_noise, gpmpc_particle_step,
gpmpc_particle_stats, gpmpc_particle_rollout; include/gpmpc.h, "Particles").  TEST INFRASTRUCTURE ONLY.

Conventions of tests/gpstate_reference.py: ``np.longdouble`` where the host has it (mpmath object arrays otherwise), the float64 Kinv is
data, the definitions are written out with none of the kernels' groupings (no tiles, no chunks, no GP groups), and every sum the GPU
tests bound by ``tol * sum |terms|`` comes back with that sum.  The normals come from tests/mppi_reference.py's Philox with the
addressing of the header: key (seed low, seed high ^ 0x50415254), counter (p, j, t, call_index), normals 2j (cosine) and 2j + 1 (sine).

A model is a dict: X (n, D), beta (n, ds), Kinv (n, n) or (ds, n, n), lam (ds, D), sf (ds,), and optionally nominal = (W (ds, D), b (ds,)),
init_cov (ds, ds), action_var (da,), process_var (ds,) (missing: the defaults 1e-3 I, float32(1e-3), 0)."""
import numpy as np

import gpstate_reference as G
import mppi_reference as MR

KEY_XOR = 0x50415254
INIT_VAR = 1e-3
ACTION_VAR = float(np.float32(1e-3))


def _sqrt(a):
    return np.frompyfunc(G._mpmath().sqrt, 1, 1)(a) if a.dtype == object else np.sqrt(a)


def dims(model):
    ds = np.asarray(model["beta"]).shape[1]
    D = np.asarray(model["X"]).shape[1]
    return ds, D - ds, D


def noise_model(model):
    ds, da, _ = dims(model)
    P = np.asarray(model.get("init_cov", np.eye(ds) * INIT_VAR), dtype=np.float64)
    av = np.asarray(model.get("action_var", np.full(da, ACTION_VAR)), dtype=np.float64).reshape(da)
    pv = np.asarray(model.get("process_var", np.zeros(ds)), dtype=np.float64).reshape(ds)
    return P, av, pv


def normals(seed, call_index, t, P, n_normals):
    """eps (P, n_normals) of step t: float64 (the GPU bound on these is absolute, 1e-12)."""
    npair = (n_normals + 1) // 2
    p, j = np.meshgrid(np.arange(P, dtype=np.uint64), np.arange(npair, dtype=np.uint64), indexing="ij")
    ctr = np.stack((p, j, np.full_like(p, t), np.full_like(p, call_index)), axis=-1)
    w = MR.philox4x32_10(ctr, (seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ KEY_XOR))
    u1, u2 = MR._uniform(w[..., 0], w[..., 1]), MR._uniform(w[..., 2], w[..., 3])
    assert np.all((u1 > 0) & (u2 > 0))
    r = np.sqrt(-2.0 * np.log(u1))
    eps = np.empty((P, 2 * npair))
    eps[:, 0::2] = r * np.cos(MR.TWO_PI * u2)
    eps[:, 1::2] = r * np.sin(MR.TWO_PI * u2)
    return eps[:, :n_normals]


def cholesky_lower(P):
    """Lower factor of a positive SEMI-definite matrix, column by column; a pivot within 16 ulp of zero (relative to the diagonal entry it
    is left of) gives a zero column.  float64, as the library computes it on the host."""
    P = np.asarray(P, dtype=np.float64)
    P = 0.5 * (P + P.T)
    ds = P.shape[0]
    L = np.zeros((ds, ds))
    big = np.abs(P).max() if ds else 0.0
    for j in range(ds):
        d = P[j, j]
        for k in range(j):
            d -= L[j, k] * L[j, k]
        if d < -1e-12 * big:
            raise ValueError("negative pivot")
        if d <= 16.0 * np.finfo(np.float64).eps * P[j, j]:
            continue
        r = np.sqrt(d)
        L[j, j] = r
        for i in range(j + 1, ds):
            s = P[i, j]
            for k in range(j):
                s -= L[i, k] * L[j, k]
            L[i, j] = s / r
    return L


def _kinv(model, a):
    K = np.asarray(model["Kinv"])
    return K if K.ndim == 2 else K[a]


def posterior(model, Z, prec=None, triangle_only=False, drop_rows_from=None):
    """m, sum |beta_i k_i|, q, sum |k_i K_ij k_j|, s2 -- each (nq, ds) in the working precision.  The two keyword arguments are
    deliberate MISTAKES for the discriminating controls: only the upper triangle of Kinv read (mirrored, as a form for symmetric matrices
    would), or its rows from an index on dropped.  (Kinv TRANSPOSED is no mistake here: k^T K k = k^T K^T k.)"""
    ds, da, D = dims(model)
    Z = np.asarray(Z, dtype=np.float64).reshape(-1, D)
    nq = Z.shape[0]
    _, _, pv = noise_model(model)
    cols = {k: [] for k in ("m", "m_abs", "q", "q_abs", "s2")}
    beta = G.cast(model["beta"], prec)
    for a in range(ds):
        ks = G.kernel(model["X"], Z, model["lam"][a], model["sf"][a], prec)        # (n, nq)
        K = G.cast(_kinv(model, a), prec)
        if triangle_only:
            K = np.triu(K) + np.triu(K, 1).T
        if drop_rows_from is not None:
            K = K.copy()
            K[drop_rows_from:, :] = K[drop_rows_from:, :] * 0
        terms = beta[:, a][:, None] * ks
        m, m_abs = terms.sum(axis=0), G._abs(terms).sum(axis=0)
        q = np.empty(nq, dtype=ks.dtype)
        q_abs = np.empty(nq, dtype=ks.dtype)
        absK = G._abs(K)
        for c in range(nq):
            k = ks[:, c]
            q[c] = k @ (K @ k)                                                  # sum_i sum_j k_i K_ij k_j: ALL entries
            q_abs[c] = G._abs(k) @ (absK @ G._abs(k))
        if "nominal" in model and model["nominal"] is not None:
            W, b = model["nominal"]
            m = m + G.cast(Z, prec) @ G.cast(np.asarray(W)[a], prec) + G.cast(np.broadcast_to(np.asarray(b, dtype=np.float64), (ds,))[a], prec)
        sf = G.cast(model["sf"][a], prec)
        for k, v in (("m", m), ("m_abs", m_abs), ("q", q), ("q_abs", q_abs), ("s2", sf * sf - q + G.cast(pv[a], prec))):
            cols[k].append(v)
    return {k: np.stack(v, axis=1) for k, v in cols.items()}


def assemble(model, x_prev, U_t, eps):
    """z (B, P, D) = (x_prev, U_t + sqrt(action_var) eps_u), float64 as the device forms it (one product, one sum)."""
    ds, da, D = dims(model)
    _, av, _ = noise_model(model)
    x_prev = np.asarray(x_prev, dtype=np.float64)
    B, P = x_prev.shape[0], x_prev.shape[1]
    z = np.empty((B, P, D))
    z[..., :ds] = x_prev
    if da:
        z[..., ds:] = np.asarray(U_t, dtype=np.float64).reshape(B, 1, da) + np.sqrt(av)[None, None, :] * np.asarray(eps)[None, :, :da]
    return z


def step(model, x_prev, U_t, eps, prec=None):
    """One step from x_prev (B, P, ds): dict(next, m, m_abs, q, q_abs, s2), each (B, P, ds) in the working precision."""
    ds, da, D = dims(model)
    z = assemble(model, x_prev, U_t, eps)
    B, P = z.shape[0], z.shape[1]
    r = {k: v.reshape(B, P, ds) for k, v in posterior(model, z.reshape(-1, D), prec).items()}
    e = G.cast(np.asarray(eps)[:, da:], prec)[None]
    s2 = r["s2"]
    pos = s2 * (s2 > 0)
    r["next"] = r["m"] + _sqrt(pos) * e
    return r


def initial(model, x0, P, seed, call_index):
    ds, _, _ = dims(model)
    L = cholesky_lower(noise_model(model)[0])
    eps = normals(seed, call_index, 0, P, ds)
    return np.asarray(x0, dtype=np.float64).reshape(-1, 1, ds) + (eps @ L.T)[None]


def rollout(model, x0, U, P, seed=0, call_index=0, prec=None):
    """particles (H+1, B, P, ds) float64 (each step evaluated in the working precision, rounded to float64), s2 (H, B, P, ds)."""
    ds, da, D = dims(model)
    U = np.asarray(U, dtype=np.float64)
    B, H = U.shape[0], U.shape[1]
    X = np.empty((H + 1, B, P, ds))
    S2 = np.empty((H, B, P, ds))
    X[0] = initial(model, x0, P, seed, call_index)
    for t in range(1, H + 1):
        r = step(model, X[t - 1], U[:, t - 1], normals(seed, call_index, t, P, da + ds), prec)
        X[t], S2[t - 1] = G.to_f64(r["next"]), G.to_f64(r["s2"])
    return X, S2


def stats(X, prec=None):
    """X (T, B, P, ds) -> mean (B, T, ds) with sum |terms|, cov (B, T, ds, ds) with sum |terms| (two-pass, divisor P - 1)."""
    X = G.cast(np.asarray(X, dtype=np.float64), prec)
    T, B, P, ds = X.shape
    mean = X.sum(axis=2) / P
    mean_abs = G._abs(X).sum(axis=2)
    d = X - mean[:, :, None, :]
    prod = d[..., :, None] * d[..., None, :]
    cov = prod.sum(axis=2) / (P - 1) if P > 1 else prod.sum(axis=2) * np.nan
    cov_abs = G._abs(prod).sum(axis=2)
    tr = lambda a: np.moveaxis(a, 0, 1)  # noqa: E731
    return {"mean": tr(mean), "mean_abs": tr(mean_abs), "cov": tr(cov), "cov_abs": tr(cov_abs)}


def violations(X, A, b):
    """X (T, B, P, ds): g (T, B, P, rows) = a_r . x - b_r in the working precision."""
    return G.cast(np.asarray(X, dtype=np.float64)) @ G.cast(np.asarray(A, dtype=np.float64)).T - G.cast(np.asarray(b, dtype=np.float64))
