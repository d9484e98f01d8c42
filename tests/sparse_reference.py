"""Extended-precision restatement of the sparse-GP (FITC) entry points: gpmpc_sparse_accumulate, gpmpc_sparse_finish,
gpmpc_sparse_append, and of the posterior they feed into the rollout.  TEST INFRASTRUCTURE ONLY.

Working precision as in tests/gpstate_reference.py: ``np.longdouble`` where the host has a 64-bit mantissa, object arrays of
``mpmath.mpf`` otherwise or on request (``prec="mp"``, at the precision mpmath is set to), and ``prec=np.float64``: the honest float64
implementation the GPU tolerances are sized against.

What is restated:
  * the whitened formulas, written out plainly, none of the device's tiles, chunks or groupings:
        Kmm = k(Z,Z) + jitter I,  L = chol(Kmm),  W = L^-1,  v_n = W k(Z, x_n),  Lambda_n = sf^2 + noise - |v_n|^2,
        G = sum_n v_n v_n^T / Lambda_n,  r = sum_n v_n y_n^T / Lambda_n,  Binv = (I + G)^-1,  alpha = W^T Binv r,  Q = W^T (I - Binv) W
    and the rank-one append of one observation;
  * the DIRECT (unwhitened) FITC definition, Sigma = (Kmm + Kmn Lambda^-1 Knm)^-1, alpha = Sigma Kmn Lambda^-1 y, Q = Kmm^-1 - Sigma
    (``direct_fitc``; meant for mpmath at >= 80 bits: its condition number is what rules it out in float64);
  * a rollout and its gradient from the pinned oracle's own pieces (``rollout``): oracle.mean_prop(...)[2] dotted with alpha and
    oracle.variance_prop(Q, ..., beta=alpha, mode="o2") inside the loop of oracle.forward_propagate, then oracle.cost, gradient by backward().

The functions take what the kernels take: the float64 W and Binv handed to a kernel are data, not something to re-derive."""
import numpy as np

from gpstate_reference import LD, HAVE_LD, MP, DEFAULT, MP_MIN_PREC, cast, kernel, to_f64, _abs, _mpmath   # noqa: F401


def _sqrt(v):
    if isinstance(v, (float, np.floating)):
        return np.sqrt(v)
    return _mpmath().sqrt(v)


def _zeros_like(A):
    return A * 0


def cholesky(A):
    """Lower Cholesky factor of a symmetric positive definite matrix, in the precision of A."""
    n = len(A)
    L = _zeros_like(A)
    for j in range(n):
        s = A[j, j]
        for k in range(j):
            s = s - L[j, k] * L[j, k]
        L[j, j] = _sqrt(s)
        for i in range(j + 1, n):
            t = A[i, j]
            if j:
                t = t - L[i, :j] @ L[j, :j]
            L[i, j] = t / L[j, j]
    return L


def tri_inv(L):
    """Explicit inverse of a lower-triangular matrix (lower triangular)."""
    n = len(L)
    W = _zeros_like(L)
    for i in range(n):
        W[i, i] = 1 / L[i, i]
        if i:
            W[i, :i] = -(L[i, :i] @ W[:i, :i]) / L[i, i]
    return W


def inv_spd(B):
    """Inverse of a symmetric positive definite matrix through its Cholesky factor: exactly symmetric up to the order of one dot product."""
    Wb = tri_inv(cholesky(B))
    Bi = Wb.T @ Wb
    return (Bi + Bi.T) / 2


def eye_like(A):
    E = _zeros_like(A)
    for i in range(len(A)):
        E[i, i] = E[i, i] + 1
    return E


def kmm(Z, lam, sf, jitter, prec=None):
    K = kernel(Z, Z, lam, sf, prec)
    jitter = cast(jitter, prec)
    for i in range(len(K)):
        K[i, i] = K[i, i] + jitter
    return K


def whiten(Z, lam, sf, jitter, prec=None):
    """W = chol(k(Z,Z) + jitter I)^-1."""
    return tri_inv(cholesky(kmm(Z, lam, sf, jitter, prec)))


def accumulate(X, Y, Z, W, lam, sf, noise, prec=None, lambda_noise=True):
    """V [M][n] = W k(Z, X), Lambda [n], G = V diag(1/Lambda) V^T, r = V diag(1/Lambda) Y for the given W.
    lambda_noise=False leaves sigma_n^2 out of Lambda (a deliberate mistake, for the discrimination tests)."""
    Kzx = kernel(Z, X, lam, sf, prec)
    W, Y, sf, noise = cast(W, prec), cast(np.asarray(Y).reshape(len(X), -1), prec), cast(sf, prec), cast(noise, prec)
    V = W @ Kzx
    kappa = sf * sf + noise if lambda_noise else sf * sf
    Lam = kappa - (V * V).sum(axis=0)
    Vw = V / Lam[None, :]
    return {"V": V, "Lambda": Lam, "G": Vw @ V.T, "r": Vw @ Y, "min_lambda": min(Lam)}


def finish(W, Binv, r, prec=None):
    """alpha = W^T Binv r, Q = W^T (I - Binv) W for the given W, Binv, r."""
    W, Binv, r = cast(W, prec), cast(Binv, prec), cast(r, prec)
    return {"alpha": W.T @ (Binv @ r), "Q": W.T @ ((eye_like(Binv) - Binv) @ W)}


def append(x, y, Z, W, lam, sf, noise, G, r, Binv, Q, prec=None):
    """One observation by the rank-one formulas; returns the updated G, r, Binv, Q, alpha and Lambda."""
    k = kernel(Z, np.asarray(x).reshape(1, -1), lam, sf, prec)[:, 0]
    W, G, r, Binv, Q, y, sf, noise = (cast(a, prec) for a in (W, G, r, Binv, Q, np.asarray(y).reshape(-1), sf, noise))
    v = W @ k
    Lam = sf * sf + noise - v @ v
    t = Binv @ v
    den = Lam + v @ t
    u = W.T @ t
    G = G + np.outer(v, v) / Lam
    r = r + np.outer(v, y) / Lam
    Binv = Binv - np.outer(t, t) / den
    Q = Q + np.outer(u, u) / den
    return {"G": G, "r": r, "Binv": Binv, "Q": Q, "alpha": W.T @ (Binv @ r), "Lambda": Lam}


def fit(X, Y, Z, lam, sf, noise, jitter, prec=None, W=None, lambda_noise=True):
    """The whole chain in the working precision: W (unless given: then it is data), G, r, Binv, alpha, Q."""
    W = whiten(Z, lam, sf, jitter, prec) if W is None else cast(W, prec)
    acc = accumulate(X, Y, Z, W, lam, sf, noise, prec, lambda_noise)
    Binv = inv_spd(eye_like(acc["G"]) + acc["G"])
    out = finish(W, Binv, acc["r"], prec)
    out.update(W=W, G=acc["G"], r=acc["r"], Binv=Binv, min_lambda=acc["min_lambda"], Lambda=acc["Lambda"])
    return out


def direct_fitc(X, Y, Z, lam, sf, noise, jitter, prec=MP):
    """The unwhitened definition: Kmm^-1, Lambda_n = sf^2 + noise - k_n^T Kmm^-1 k_n, Sigma = (Kmm + Kmn Lambda^-1 Knm)^-1,
    alpha = Sigma Kmn Lambda^-1 y, Q = Kmm^-1 - Sigma."""
    Km = kmm(Z, lam, sf, jitter, prec)
    Kmn = kernel(Z, X, lam, sf, prec)
    Y, sf, noise = cast(np.asarray(Y).reshape(len(X), -1), prec), cast(sf, prec), cast(noise, prec)
    Kmi = inv_spd(Km)
    Lam = sf * sf + noise - ((Kmi @ Kmn) * Kmn).sum(axis=0)
    Kw = Kmn / Lam[None, :]
    Sigma = inv_spd(Km + Kw @ Kmn.T)
    return {"alpha": Sigma @ (Kw @ Y), "Q": Kmi - Sigma, "Lambda": Lam}


def predict(Z, alpha, Q, lam, sf, Xs, prec=None):
    """mean [p][n_targets] = k_*^T alpha, var [p] = sf^2 - k_*^T Q k_*."""
    Ks = kernel(Xs, Z, lam, sf, prec)
    alpha, Q, sf = cast(alpha, prec), cast(Q, prec), cast(sf, prec)
    return Ks @ alpha, sf * sf - ((Ks @ Q) * Ks).sum(axis=1)


def max_abs(a):
    a = np.asarray(a)
    return float(max(_abs(a).reshape(-1))) if a.size else 0.0


def err(a, b):
    """max |a - b|, evaluated in the wider of the two precisions."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == object or b.dtype == object:
        a, b = cast(a, MP), cast(b, MP)
    elif a.dtype != b.dtype:
        a, b = a.astype(LD), b.astype(LD)
    return max_abs(a - b)


# ------------------------------------------------------------------------------------------------------------------ problems
def problem(seed, n, M, D, n_targets, sigma_n=0.1, lam_range=(0.7, 2.5), sf=1.2, jitter=None):
    """Kernel-level test inputs, float64: X ~ U(-2, 2) [n][D], Y [n][n_targets] smooth + noise, Z a random subset of X plus a small
    displacement (or fresh draws where M > n), lambda ~ U(lam_range), W = chol(Kmm)^-1 rounded from the long double evaluation and
    Binv = (I + G)^-1 likewise (symmetric): data to the kernels.  Also one further observation (xnew, ynew)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (n, D))
    Y = np.stack([np.sin(X * (a + 1)).sum(axis=1) for a in range(n_targets)], axis=1) + sigma_n * rng.standard_normal((n, n_targets))
    Z = rng.uniform(-2, 2, (M, D))
    k = min(n, M)
    Z[:k] = X[rng.choice(n, size=k, replace=False)] + 1e-3 * rng.standard_normal((k, D))
    lam = rng.uniform(lam_range[0], lam_range[1], D)
    noise = sigma_n ** 2
    jitter = 1e-6 * sf * sf if jitter is None else jitter
    W = to_f64(whiten(Z, lam, sf, jitter))
    ref = fit(X, Y, Z, lam, sf, noise, jitter, W=W)
    Binv = to_f64(ref["Binv"])
    Binv = (Binv + Binv.T) / 2
    out = {"n": n, "M": M, "D": D, "nt": n_targets, "X": X, "Y": Y, "Z": Z, "lam": lam, "sf": sf, "noise": noise, "jitter": jitter,
           "W": W, "Binv": Binv, "xnew": rng.uniform(-2, 2, D), "ynew": rng.standard_normal(n_targets)}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# Shape ladder of the GPU tests: one either side of every 16-deep stage and 64-wide tile of the kernels, a second and a third tile
# (M = 130), M = 1; n either side of a 64-row chunk edge, and three full chunks and a partial one (n = 200 at chunk 64).
LADDER_M = (1, 15, 16, 17, 33, 64, 65, 130)
LADDER_N = (1, 63, 64, 65, 200)
LADDER_D = (2, 5, 8)


def ladder():
    """[(M, n, D, n_targets)]: D and n_targets cycle over the ladder so that every value meets small and large M and n."""
    out = []
    for i, M in enumerate(LADDER_M):
        for j, n in enumerate(LADDER_N):
            out.append((M, n, LADDER_D[(i + j) % 3], (1, 4)[(i + j // 2) % 2]))
    return out


def seed_of(M, n, D, nt):
    return ((M * 1000 + n) * 10 + D) * 10 + nt


def allowance(ref_ld, ref_f64):
    """The device's allowance for one output array: max(8 e64, 1e-13 max|array|), e64 the max-abs error of the float64 evaluation of the
    reference against its extended-precision one on the same inputs.  (The x8: the float64 error moves by less than x2 across data
    orders and chunk sizes -- it is set by W, not by the summation order -- plus a different tiling.)"""
    return max(8.0 * err(ref_f64, ref_ld), 1e-13 * max_abs(ref_ld))


# ------------------------------------------------------------------------------------------------------------------ rollout
def rollout(Z, alpha, Q, lam, sf, H, x0, U, Qc, Rc, gamma, x_ref=None, u_ref=None, fullcov=False, want_grad=True):
    """The oracle's rollout on a posterior given as (Z, alpha [M][ds], Q [ds][M][M] or [M][M]): the loop of oracle.forward_propagate
    (forward_propagate_fullcov with ``fullcov``) with mean l . alpha and oracle.variance_prop(Q, ..., beta=alpha, mode="o2"), then
    oracle.cost and backward().  float64 torch, as the oracle."""
    import torch
    from oracle import gpmpc_oracle as O
    Zt, At, lamt = O._t(Z), O._t(alpha), O._t(np.asarray(lam))
    ds, D = At.shape[1], Zt.shape[1]
    da = D - ds
    Qt = O._t(Q)
    if Qt.dim() == 2:
        Qt = Qt.unsqueeze(0).expand(ds, -1, -1)
    sf = [float(v) for v in np.broadcast_to(np.asarray(sf, dtype=np.float64).reshape(-1), (ds,))]
    x_ref = np.zeros(ds) if x_ref is None else x_ref
    u_ref = np.zeros(da) if u_ref is None else u_ref
    Ut = O._t(U).clone().reshape(H, da).requires_grad_(want_grad)
    means = [O._t(x0)]
    covs = [O.INIT_STATE_VAR * torch.eye(ds, dtype=O.F64)]
    for t in range(1, H + 1):
        u = torch.cat((means[t - 1], Ut[t - 1, :]))
        S = torch.zeros((D, D), dtype=O.F64)
        S[:ds, :ds] = covs[t - 1]
        S = S + torch.diag(torch.cat((torch.zeros(ds, dtype=O.F64), torch.full((da,), O.ACTION_NOISE_VAR, dtype=O.F64))))
        mu_t = []
        rows = [[torch.zeros((), dtype=O.F64)] * ds for _ in range(ds)]
        for a in range(ds):
            l = O.mean_prop(Qt[a], lamt[a], u, S, Zt, At[:, a], sf[a])[2]
            m = torch.dot(At[:, a], l)
            rows[a][a] = O.variance_prop(Qt[a], lamt[a], u, S, Zt, m, At[:, a], sf[a], mode="o2")
            mu_t.append(m)
        if fullcov:
            for a in range(ds):
                for b in range(a + 1, ds):
                    c = O.covariance_prop(lamt[a], lamt[b], u, S, Zt, mu_t[a], mu_t[b], At[:, a], At[:, b], sf[a], sf[b], bug_compatible=False)
                    rows[a][b] = c
                    rows[b][a] = c
        means.append(torch.stack(mu_t))
        covs.append(torch.stack([torch.stack(r) for r in rows]))
    c = O.cost(means, Ut, covs, O._t(x_ref), O._t(u_ref), Qc, Rc, gamma)
    out = {"cost": float(c.item()), "means": torch.stack([m.detach() for m in means]).numpy(),
           "covs": torch.stack([s.detach() for s in covs]).numpy()}
    out["vars"] = np.stack([np.diag(s) for s in out["covs"]])
    if want_grad:
        c.backward()
        out["grad"] = Ut.grad.detach().numpy().copy()
    return out


def fit_bundle(pb, Z, jitter=None, prec=None, lambda_noise=True):
    """(alpha [M][ds], Q [ds][M][M]) of a synth_problem dict, one whitened fit per GP (their length-scales differ), float64 arrays rounded
    from the working precision.  jitter None: 1e-6 sigma_f^2."""
    ds = pb["Y"].shape[1]
    alpha, Q = [], []
    for a in range(ds):
        sf, sn = float(pb["sigma_f"][a]), float(pb["sigma_n"][a])
        f = fit(pb["X"], pb["Y"][:, a], Z, pb["lambdas"][a], sf, sn * sn, 1e-6 * sf * sf if jitter is None else jitter, prec,
                lambda_noise=lambda_noise)
        alpha.append(to_f64(f["alpha"])[:, 0])
        Q.append(to_f64(f["Q"]))
    return np.stack(alpha, axis=1), np.stack(Q)
