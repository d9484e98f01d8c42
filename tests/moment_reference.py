"""Reference, units, float64 emulation and input tables for SINGLE-STEP moment matching with a full input covariance
(gpmpc_moment_match: csrc/moment.hip, csrc/moment_dev.h) -- shared by tests/test_host_moment.py and tests/test_gpu_moment.py.

Reference.  Values (mean, cov with the variances on its diagonal, l) from the long double build of oracle/cport/gpmpc_cpu_given.c, Jacobians
from its long double COMPLEX build by the complex step (h = 1e-20, one run per u_k and one per pair k <= l along (E_kl + E_lk)/2), both on the
constants the kernels read (GPPack.beta() / GPPack.weights()) and at sym(S), which is what the kernels read.  `mp_step` restates the same
formulas in mpmath at 50 digits from src/tools/uncertainty_prop.py:296-465 (inverse and determinant from mpmath, no Cholesky, no h-space, no
elimination of our own) with central differences at 50 digits; it pins the complex-step entries at N <= 6, D <= 3 (tests/test_host_moment.py).

Units.  K = |got - reference| / (2^-53 A), one A per output entry: the sum of the absolute values of the terms the entry is formed from,
each term e^q weighted with om = 1 + (the absolute terms of its exponent q): A_mean, A_var, A_cov of gpmpc_cpu_given.c without that
weight were off by 10 ... 560 for a query six length-scales from the data.  With |.| entry-wise, B = (S + Lambda)^-1, Mm = S + Lambda,
Bc = |B||Mm||B| (what an elimination loses of B entry by entry, as W in the cost budget: with |B| alone kappa(S + Lambda) > 1e3 was off by up
to 1200), v_i = u - x_i, f1 = |B||v_i|, f2 = Bc |v_i|, om_i = 1 + 1/2 |v_i|^T Bc |v_i|, w_i = c_m |beta_i| l_i:
    l_i          c_m l_i om_i                                   mean         sum_i w_i om_i
    dmean/du_k   sum_i w_i (om_i f1 + f2)_k                     (the product rule of the term: its exponent and its factor B v_i)
    dmean/dS_kl  1/2 sum_i w_i [om_i (|B| + f1 f1^T) + Bc + f1 f2^T + f2 f1^T]_kl
    var, dvar    the same over the pairs i <= j with A = (S + Lambda/2)^-1, s_ij = v_i + v_j, |M_ij| E_ij for w and the factors 1/4, 1/8,
                 plus sf^2 (var) and the product rule of mu^2: 2 (A_mean |dmu| + |mu| A_dmu)
    cov, dcov    the same over all (i, j) with K |beta_a,i beta_b,j| E_ij, Am = R^-1 S (conditioned: |Ri||R||Ri| |S|), P1, P2, C of
                 k_cross_cov term-wise, R^-T Gabs R^-1 and the dK term with |Ri| and |Ri||R||Ri|, plus the product rule of mu_a mu_b
Bc is a bound, not an estimate: at kappa > 1e3 (the stiff family) the sums come out 1e2 ... 1e5 times more exact than it allows.
The units need three digits, so they are computed in float64 from the float64 inverse; no sum below 2^-960 counts (TINY: its terms are
subnormal, not relatively rounded).

Emulation.  `emulate` restates in numpy float64 the formulas AS THE KERNELS WRITE THEM: B and A by Gauss-Jordan without pivoting, the Cholesky
factor Cm of A/8, the h-space moments Z0 / Z1 / Z2 with the expanded exponent, dT/dS = -1/2 T A + 8 c Cm^T Z2 Cm, the Gaussian-product cross
units of the pair kernel (cross="pair") and k_cross_cov's P1 / P2 / C / dK algebra in both forms (cross="direct").  K_ref is its K; its
`defect` switch is where the defects of the table in tests/test_host_moment.py are emulated.
"""
import numpy as np

LD = np.longdouble
TINY = 2.0 ** -960

INSTANCES = [(1, 1), (2, 2), (3, 2), (4, 3), (5, 4), (6, 3), (7, 2), (8, 1), (8, 8)]
EDGE_N = [1, 63, 64, 65, 130, 257]                 # at (3, 2): the 64-column staging and 256-row trips of k_cross_cov, out_l's second row
LARGE = [(3, 1, 2100), (6, 1, 1100)]               # a second trip of the mean loop (base += 2 RB 256: RB = 4 at D <= 5, else 2)
N_DEFAULT = 90
FAMILIES = ("generic", "correlated", "zero", "zero_row", "far", "skew", "stiff")
DEFECTS = ("dvar_dS_gp1", "no_amplitudes", "no_mean_terms_dS", "z_for_zt", "factor_4_for_2", "rel_1e-5", "l_row_256")

OUTPUTS = ("mean", "var", "cov", "l", "dmean_du", "dmean_dS", "dvar_du", "dvar_dS", "dcov_du", "dcov_dS")


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def problem(D, ds, N, seed=0):
    """A GP problem in the keys oracle.cport reads: amplitudes from [0.6, 1.8], length-scales distinct per GP from [0.3, 5]."""
    rng = np.random.default_rng([D, ds, N, seed])
    X = rng.normal(size=(N, D))
    lam = rng.uniform(0.3, 5.0, size=(ds, D))
    sf = rng.uniform(0.6, 1.8, size=ds)
    sn = np.full(ds, 0.1)
    Y = np.stack([sf[a] * (np.sin(X @ rng.normal(size=D)) + 0.1 * rng.normal(size=N)) for a in range(ds)], axis=1)
    Kinv = np.zeros((ds, N, N))
    for a in range(ds):
        d2 = ((X[:, None, :] - X[None, :, :]) ** 2 / lam[a]).sum(-1)
        Kinv[a] = np.linalg.inv(sf[a] ** 2 * np.exp(-0.5 * d2) + sn[a] ** 2 * np.eye(N))
    return {"X": X, "Y": Y, "lambdas": lam, "sigma_f": sf, "sigma_n": sn, "ds": ds, "da": D - ds, "Ky_inv": Kinv}


def queries(pb, family, nq, seed=0):
    """u (nq, D), S (nq, D, D) of one input family (FAMILIES)."""
    X, lam = pb["X"], pb["lambdas"]
    D = X.shape[1]
    rng = np.random.default_rng([D, pb["ds"], FAMILIES.index(family), seed])
    u = 0.5 * rng.normal(size=(nq, D))
    S = np.zeros((nq, D, D))
    for q in range(nq):
        A = rng.normal(size=(D, D))
        gen = 0.02 * A @ A.T + 0.01 * np.eye(D)
        if family in ("generic", "far", "skew"):
            S[q] = gen
        elif family == "correlated":                           # rho = 0.95 at a scale of half the mean length-scale
            s = 0.5 * lam.mean()
            S[q] = s * (0.95 * np.ones((D, D)) + 0.05 * np.eye(D))
        elif family == "zero_row":
            S[q] = gen
            S[q, 0, :] = 0.0
            S[q, :, 0] = 0.0
        elif family == "stiff":                                # kappa(S + Lambda) >= 1e4 / 5
            w = rng.normal(size=D)
            w /= np.linalg.norm(w)
            S[q] = 1e4 * np.outer(w, w) + 0.01 * np.eye(D)
        if family == "skew":                                   # stored non-symmetric: the kernels read (S + S^T)/2
            G = rng.normal(size=(D, D))
            S[q] += 1e-3 * (G - G.T)
        if family == "far":                                    # six length-scales (of the widest GP) beyond the data, along the axis
            k = int(np.argmin(lam.max(0) / lam.min(0)))        # where the GPs' length-scales differ least
            u[q, k] = X[:, k].max() + 6.0 * np.sqrt(lam[:, k].max() + gen[k, k])
    return u, S


def bug_held(family, N):
    """Whether a call of this family holds the bug-compatible FORM: at S = 0 (Am = 0) and at N = 1 the two forms are the same number, and
    in the stiff family they differ by less than 1e6 of its (bounding) units; elsewhere by more (tests/test_host_moment.py asserts it)."""
    return N > 1 and family not in ("zero", "stiff")


def sym(S):
    return 0.5 * (S + np.swapaxes(S, -1, -2))


def upper_weights(W, a, N):
    """The pair weights of GP a as an upper-triangular (i <= j) matrix, off-diagonal pairs doubled (GPPack.weights() layout)."""
    return np.asarray(W[a], dtype=np.float64)[:N, :N].T


# ------------------------------------------------------------------------------------------------------------------------------
# units (float64; see the header)
# ------------------------------------------------------------------------------------------------------------------------------
def _cross_terms(X, u, S, la, lb, bug):
    d = X - u
    L = 1.0 / la + 1.0 / lb
    R = S * L[None, :] + np.eye(len(u))
    Ri = np.linalg.inv(R)
    Am = Ri @ S
    p, r = d / la, d / lb
    pc, rc = (r, p) if bug else (p, r)
    al = -0.5 * (d * p).sum(1) + 0.5 * ((p @ Am.T) * p).sum(1)
    ga = -0.5 * (d * r).sum(1) + 0.5 * ((r @ Am.T) * r).sum(1)
    E = np.exp(al[:, None] + ga[None, :] + (pc @ Am) @ rc.T)
    return d, L, R, Ri, Am, p, r, pc, rc, E


def units(pb, beta, W, u, S, bug, val, jac, want_var=True):
    """A per entry for one query: u (D,), S (D, D) symmetric; val / jac: the reference values of this query (for the product rules)."""
    X, lam, sf = pb["X"], pb["lambdas"], pb["sigma_f"]
    N, D = X.shape
    ds = pb["ds"]
    beta = np.asarray(beta, dtype=np.float64)[:, :N]
    v = u - X
    out = {k: None for k in OUTPUTS}
    A_mean, A_cov = np.zeros(ds), np.zeros((ds, ds))
    out["l"] = np.zeros((ds, N))
    A_du, A_dS = np.zeros((ds, D)), np.zeros((ds, D, D))
    Av_du, Av_dS = np.zeros((ds, D)), np.zeros((ds, D, D))
    mu, dmu_u, dmu_S = val["mean"], jac["dmean_du"], jac["dmean_dS"]
    for a in range(ds):
        Mm = S + np.diag(lam[a])
        B = np.linalg.inv(Mm)
        cm = sf[a] ** 2 / np.sqrt(np.linalg.det(S / lam[a][:, None] + np.eye(D)))
        l = np.exp(-0.5 * ((v @ B.T) * v).sum(1))
        aB, Bc = np.abs(B), np.abs(B) @ np.abs(Mm) @ np.abs(B)
        f1, f2 = np.abs(v) @ aB.T, np.abs(v) @ Bc.T            # |B||v_i| and what the inverse can lose of it
        om = 1.0 + 0.5 * (f2 * np.abs(v)).sum(1)               # weight of a term: one plus what its exponent can lose
        out["l"][a] = cm * l * om
        w = cm * np.abs(beta[a]) * l
        wo = w * om
        A_mean[a] = wo.sum()
        A_du[a] = wo @ f1 + w @ f2
        F12 = (f1 * w[:, None]).T @ f2
        A_dS[a] = 0.5 * (wo.sum() * aB + (f1 * wo[:, None]).T @ f1 + w.sum() * Bc + F12 + F12.T)
        if not want_var:
            continue
        Ma = S + 0.5 * np.diag(lam[a])
        A = np.linalg.inv(Ma)
        c = 1.0 / np.sqrt(np.linalg.det(2.0 * S / lam[a][:, None] + np.eye(D)))
        s = v[:, None, :] + v[None, :, :]
        aA, Ac = np.abs(A), np.abs(A) @ np.abs(Ma) @ np.abs(A)
        g1, g2 = np.abs(s) @ aA.T, np.abs(s) @ Ac.T
        P = c * np.abs(upper_weights(W, a, N)) * np.exp(-0.125 * np.einsum("ijk,kl,ijl->ij", s, A, s))
        Po = P * (1.0 + 0.125 * (g2 * np.abs(s)).sum(-1))
        A_cov[a, a] = sf[a] ** 2 + Po.sum() + 2.0 * A_mean[a] * abs(mu[a])
        Av_du[a] = (0.25 * (np.einsum("ij,ijk->k", Po, g1) + np.einsum("ij,ijk->k", P, g2))
                    + 2.0 * (A_mean[a] * abs(dmu_u[a]) + abs(mu[a]) * A_du[a]))
        G12 = np.einsum("ij,ijk,ijl->kl", P, g1, g2)
        Av_dS[a] = (0.5 * (Po.sum() * aA + P.sum() * Ac) + 0.125 * (np.einsum("ij,ijk,ijl->kl", Po, g1, g1) + G12 + G12.T)
                    + 2.0 * (A_mean[a] * abs(dmu_S[a]) + abs(mu[a]) * A_dS[a]))
    out["mean"], out["dmean_du"], out["dmean_dS"] = A_mean, A_du, A_dS
    if not want_var:
        return out
    out["var"] = np.diagonal(A_cov).copy()
    out["dvar_du"], out["dvar_dS"] = Av_du, Av_dS
    Ac_du, Ac_dS = np.zeros((ds, ds, D)), np.zeros((ds, ds, D, D))
    for a in range(ds):
        Ac_du[a, a], Ac_dS[a, a] = Av_du[a], Av_dS[a]
        for b in range(ds):
            if a == b or (not bug and b < a):
                continue
            la, lb = lam[a], lam[b]
            d, L, R, Ri, Am, p, r, pc, rc, E = _cross_terms(X, u, S, la, lb, bug)
            K = (sf[a] * sf[b]) ** 2 / np.sqrt(np.linalg.det(R))
            aRi = np.abs(Ri)
            Rc = aRi @ np.abs(R) @ aRi
            aAm = np.abs(Am)
            cAm = Rc @ np.abs(S)                               # what the inverse can lose of Am = R^-1 S
            cAm = 0.5 * (cAm + cAm.T)
            ap, ar, apc, arc, ad = np.abs(p), np.abs(r), np.abs(pc), np.abs(rc), np.abs(d)
            om = (1.0 + 0.5 * ((ad * ap).sum(1) + ((ap @ cAm) * ap).sum(1))[:, None] + 0.5 * ((ad * ar).sum(1) + ((ar @ cAm) * ar).sum(1))[None, :]
                  + (apc @ cAm) @ arc.T)
            P = K * np.abs(beta[a])[:, None] * np.abs(beta[b])[None, :] * E
            Po = P * om
            A_cov[a, b] = Po.sum() + A_mean[a] * abs(mu[b]) + A_mean[b] * abs(mu[a])
            lp, lr = (1.0 / lb, 1.0 / la) if bug else (1.0 / la, 1.0 / lb)
            prod_u = (A_mean[a] * abs(dmu_u[b]) + abs(mu[a]) * A_du[b] + A_mean[b] * abs(dmu_u[a]) + abs(mu[b]) * A_du[a])
            Ac_du[a, b] = prod_u
            for Pw, am, dg in ((Po, aAm, 1.0), (P, cAm, 0.0)):          # the terms with their weights; the terms' own matrices
                aP1 = am / la[:, None] / la[None, :] + dg * np.diag(1.0 / la)
                aP2 = am / lb[:, None] / lb[None, :] + dg * np.diag(1.0 / lb)
                aC = lp[:, None] * am * lr[None, :]
                Ac_du[a, b] = Ac_du[a, b] + (Pw.sum(1) @ ad) @ (aP1 + aC.T).T + (Pw.sum(0) @ ad) @ (aP2 + aC).T

            def gabs(Pw):
                X1 = apc.T @ Pw @ arc
                return 0.5 * (ap * Pw.sum(1)[:, None]).T @ ap + 0.5 * (ar * Pw.sum(0)[:, None]).T @ ar + 0.5 * (X1 + X1.T)
            Go, Gp = gabs(Po), gabs(P)
            T = aRi.T @ Go @ aRi + Rc.T @ Gp @ aRi + aRi.T @ Gp @ Rc
            LR = L[:, None] * (Po.sum() * aRi + P.sum() * Rc)
            prod_S = (A_mean[a] * abs(dmu_S[b]) + abs(mu[a]) * A_dS[b] + A_mean[b] * abs(dmu_S[a]) + abs(mu[b]) * A_dS[a])
            Ac_dS[a, b] = 0.5 * (T + T.T) + 0.25 * (LR + LR.T) + prod_S
            if not bug:
                A_cov[b, a], Ac_du[b, a], Ac_dS[b, a] = A_cov[a, b], Ac_du[a, b], Ac_dS[a, b]
    out["cov"], out["dcov_du"], out["dcov_dS"] = A_cov, Ac_du, Ac_dS
    return out


def reference(pb, beta, W, u, S, bug=False, nthreads=8, want_var=True):
    """Long double reference and units of nq queries: (ref, A), dicts over OUTPUTS of arrays with the leading axis nq; taken at sym(S).
    want_var=False (the large-N cases): the variance side of the units is left out (None); the values are all there."""
    from oracle import cport
    u = np.asarray(u, dtype=np.float64).reshape(-1, pb["X"].shape[1])
    Ss = sym(np.asarray(S, dtype=np.float64).reshape(u.shape[0], u.shape[1], u.shape[1]))
    val = cport.given_step_full(pb, beta, W, u, Ss, prec="ld", nthreads=nthreads, bug=bug, want_l=True)
    jac = cport.given_step_full_jac(pb, beta, W, u, Ss, prec="cld", nthreads=nthreads, bug=bug)
    ref = {"mean": val["mean"], "cov": val["cov"], "var": np.diagonal(val["cov"], axis1=1, axis2=2).copy(), "l": val["l"],
           "dmean_du": jac["dmean_du"], "dmean_dS": jac["dmean_dS"], "dcov_du": jac["dcov_du"], "dcov_dS": jac["dcov_dS"],
           "dvar_du": np.stack([np.stack([jac["dcov_du"][q, a, a] for a in range(pb["ds"])]) for q in range(u.shape[0])]),
           "dvar_dS": np.stack([np.stack([jac["dcov_dS"][q, a, a] for a in range(pb["ds"])]) for q in range(u.shape[0])])}
    per_q = [units(pb, beta, W, u[q], Ss[q], bug, {k: x[q] for k, x in val.items()}, {k: x[q] for k, x in jac.items()}, want_var)
             for q in range(u.shape[0])]
    A = {k: (None if per_q[0][k] is None else np.stack([p[k] for p in per_q])) for k in OUTPUTS}
    return ref, A


def k_of(got, ref, A):
    """max over the entries of |got - ref| / (2^-53 max(A, TINY)); NaN or inf anywhere in `got` gives inf."""
    got, ref, A = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(A, dtype=np.float64)
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    if got.size == 0:
        return 0.0
    if not np.all(np.isfinite(got)):
        return float("inf")
    return float(np.max(np.abs(got.astype(LD) - ref.astype(LD)) / (LD(2.0 ** -53) * np.maximum(A, TINY).astype(LD))))


# ------------------------------------------------------------------------------------------------------------------------------
# float64 emulation of the kernels' formulas
# ------------------------------------------------------------------------------------------------------------------------------
def gj_nopivot(M):
    """Inverse and determinant by Gauss-Jordan WITHOUT pivoting, step for step as lds_inverse_pair (moment_dev.h)."""
    n = M.shape[0]
    a, iv, det = M.astype(np.float64).copy(), np.eye(n), 1.0
    for k in range(n):
        pv = a[k, k]
        ip = 1.0 / pv
        det *= pv
        akc, ikc = a[k] * ip, iv[k] * ip
        f = a[:, k].copy()
        a, iv = a - np.outer(f, akc), iv - np.outer(f, ikc)
        a[k], iv[k] = akc, ikc
    return iv, det


def chol_upper(Am, scale):
    """Upper-triangular Cm with Cm^T Cm = scale sym(Am): lds_cholesky_upper."""
    n = Am.shape[0]
    L = np.zeros((n, n))
    for c in range(n):
        L[c, c] = np.sqrt(scale * Am[c, c] - (L[c, :c] ** 2).sum())
        for r in range(c + 1, n):
            L[r, c] = (scale * 0.5 * (Am[r, c] + Am[c, r]) - (L[r, :c] * L[c, :c]).sum()) / L[c, c]
    return L.T.copy()


def _hspace(Wu, hr, hc):
    """Z0, Z1, Z2 of sum_ij Wu_ij exp(-|hr_i + hc_j|^2) (1, h, h h^T), h = hr_i + hc_j, the exponent expanded as the pair kernels do."""
    E = Wu * np.exp(-((hr * hr).sum(1)[:, None] + (hc * hc).sum(1)[None, :] + 2.0 * hr @ hc.T))
    h = hr[:, None, :] + hc[None, :, :]
    return E.sum(), np.einsum("ij,ijk->k", E, h), np.einsum("ij,ijk,ijl->kl", E, h, h)


def emulate(pb, beta, W, u, S, bug=False, cross="direct", defect=None, want_var=True):
    """One query in float64 as the kernels write it; dict over OUTPUTS.  cross: "pair" (Gaussian-product cross units, consistent form
    only) | "direct" (k_cross_cov).  defect: one of DEFECTS or None.  want_var=False: the mean side only (the large-N cases)."""
    X, lam, sf = pb["X"], pb["lambdas"], pb["sigma_f"]
    N, D = X.shape
    ds = pb["ds"]
    beta = np.asarray(beta, dtype=np.float64)[:, :N]
    S = sym(np.asarray(S, dtype=np.float64))
    assert not (bug and cross == "pair")
    o = {"mean": np.zeros(ds), "var": np.zeros(ds), "cov": np.zeros((ds, ds)), "l": np.zeros((ds, N)),
         "dmean_du": np.zeros((ds, D)), "dmean_dS": np.zeros((ds, D, D)), "dvar_du": np.zeros((ds, D)), "dvar_dS": np.zeros((ds, D, D)),
         "dcov_du": np.zeros((ds, ds, D)), "dcov_dS": np.zeros((ds, ds, D, D))}
    d = u - X
    for a in range(ds):
        B, det0 = gj_nopivot(S + np.diag(lam[a]))
        Am, det1 = gj_nopivot(S + 0.5 * np.diag(lam[a]))
        cm = sf[a] ** 2 / np.sqrt(det0 / np.prod(lam[a]))
        c = 1.0 / np.sqrt(det1 / np.prod(0.5 * lam[a]))
        Cm = chol_upper(Am, 0.125)
        ex = np.exp(-0.5 * ((d @ B.T) * d).sum(1))
        o["l"][a] = cm * ex
        p = beta[a] * ex
        S0, S1, S2 = p.sum(), p @ d, (d * p[:, None]).T @ d
        mu = cm * S0
        dmu_du = -cm * (B @ S1)
        dmu_dS = -0.5 * mu * B + 0.5 * cm * ((B @ S2) @ B)
        o["mean"][a], o["dmean_du"][a], o["dmean_dS"][a] = mu, dmu_du, dmu_dS
        if not want_var:
            continue
        h = d @ Cm.T
        Z0, Z1, Z2 = _hspace(upper_weights(W, a, N), h, h)
        T = c * Z0
        o["mean"][a], o["var"][a] = mu, sf[a] ** 2 - T - mu * mu
        o["cov"][a, a] = o["var"][a]
        dT_du = -4.0 * c * (Cm.T @ Z1)
        dT_dS = -0.5 * T * Am + 8.0 * c * (Cm.T @ (Z2 @ Cm))
        if defect == "dvar_dS_gp1" and a == 1:               # GP 1 alone: an ANTISYMMETRIC error of 1e-3 (the derivative taken as if
            sgn = np.triu(np.ones((D, D)), 1) - np.tril(np.ones((D, D)), -1)      # S_kl and S_lk were independent, say): no symmetric
            dT_dS = dT_dS + 1e-3 * np.abs(dT_dS).max() * sgn                      # direction and no rollout sees it
        o["dmean_du"][a], o["dmean_dS"][a] = dmu_du, dmu_dS
        o["dvar_du"][a], o["dvar_dS"][a] = -dT_du - 2.0 * mu * dmu_du, -dT_dS - 2.0 * mu * dmu_dS
        o["dcov_du"][a, a], o["dcov_dS"][a, a] = o["dvar_du"][a], o["dvar_dS"][a]
    for a in range(ds if want_var else 0):
        for b in range(ds):
            if a == b or (not bug and b < a):
                continue
            la, lb = lam[a], lam[b]
            mua, mub = o["mean"][a], o["mean"][b]
            amp = (sf[a] * sf[b]) if defect == "no_amplitudes" else (sf[a] * sf[b]) ** 2
            if cross == "pair":
                lab = la * lb / (la + lb)
                Bab, det = gj_nopivot(S + np.diag(lab))
                c = np.sqrt(np.prod(lab) / det)
                Cm = chol_upper(Bab, 0.5)
                wa, wb = lb / (la + lb), la / (la + lb)
                dx = X[:, None, :] - X[None, :, :]
                Wab = amp * beta[a][:, None] * beta[b][None, :] * np.exp(-0.5 * (dx * dx / (la + lb)).sum(-1))
                Z0, Z1, Z2 = _hspace(Wab, (d * wa) @ Cm.T, (d * wb) @ Cm.T)
                F = c * Z0
                cov = F - mua * mub
                fu = -4.0 if defect == "factor_4_for_2" else -2.0
                du = fu * c * (Cm.T @ Z1) - mub * o["dmean_du"][a] - mua * o["dmean_du"][b]
                dS = -0.5 * F * Bab + 2.0 * c * (Cm.T @ (Z2 @ Cm))
                if defect != "no_mean_terms_dS":
                    dS = dS - mub * o["dmean_dS"][a] - mua * o["dmean_dS"][b]
            else:
                dd, L, R, _, _, p, r, pc, rc, _ = _cross_terms(X, u, S, la, lb, bug)
                Ri, det = gj_nopivot(R)             # (the kernel pivots: small_inverse; R = S L + I of a covariance S never asks for it)
                Am = Ri @ S
                al = -0.5 * (dd * p).sum(1) + 0.5 * ((p @ Am.T) * p).sum(1)
                ga = -0.5 * (dd * r).sum(1) + 0.5 * ((r @ Am.T) * r).sum(1)
                e = beta[a][:, None] * beta[b][None, :] * np.exp(al[:, None] + ga[None, :] + (pc @ Am) @ rc.T)
                W0 = e.sum()
                K = amp / np.sqrt(det)
                cov = K * W0 - mua * mub
                mi, mj = e.sum(1) @ dd, e.sum(0) @ dd
                P1 = Am / la[:, None] / la[None, :] - np.diag(1.0 / la)
                P2 = Am / lb[:, None] / lb[None, :] - np.diag(1.0 / lb)
                lp, lr = (1.0 / lb, 1.0 / la) if bug else (1.0 / la, 1.0 / lb)
                C = lp[:, None] * Am * lr[None, :]
                du = -K * (P1 @ mi + P2 @ mj + C @ mj + C.T @ mi) - o["dmean_du"][a] * mub - mua * o["dmean_du"][b]
                X1 = pc.T @ e @ rc
                G = 0.5 * (p * e.sum(1)[:, None]).T @ p + 0.5 * (r * e.sum(0)[:, None]).T @ r + 0.5 * (X1 + X1.T)
                T2 = (Ri if defect == "z_for_zt" else Ri.T) @ G @ Ri
                LR = L[:, None] * Ri
                dS = 0.5 * K * (T2 + T2.T) - 0.25 * K * (LR + LR.T) * W0
                if defect != "no_mean_terms_dS":
                    dS = dS - o["dmean_dS"][a] * mub - mua * o["dmean_dS"][b]
            o["cov"][a, b], o["dcov_du"][a, b], o["dcov_dS"][a, b] = cov, du, dS
            if not bug:
                o["cov"][b, a], o["dcov_du"][b, a], o["dcov_dS"][b, a] = cov, du, dS
    if defect == "rel_1e-5":
        for k in ("dmean_du", "dmean_dS", "dvar_du", "dvar_dS"):      # (in the off-diagonal dcov g2's 1e-6 band would see it)
            o[k] = o[k] * (1.0 + 1e-5)
        for a in range(ds):
            o["dcov_du"][a, a], o["dcov_dS"][a, a] = o["dvar_du"][a], o["dvar_dS"][a]
    if defect == "l_row_256" and N > 256:                      # out_l's second row of a trip written to the first
        o["l"][:, :N - 256] = o["l"][:, 256:].copy()
    return o


def k_all(got, ref, A, q, outputs=OUTPUTS):
    """{output: K} of one query q of a reference (ref, A)."""
    return {k: k_of(got[k], ref[k][q], A[k][q]) for k in outputs if A[k] is not None and k in got}


# ------------------------------------------------------------------------------------------------------------------------------
# mpmath restatement (N <= 6, D <= 3)
# ------------------------------------------------------------------------------------------------------------------------------
def mp_step(pb, beta, W, u, S, bug=False, dps=50):
    """mean (ds,), cov (ds, ds), l (ds, N) and the Jacobians (central differences at `dps` digits, symmetric directions in S) of one query,
    from the direct formulas of src/tools/uncertainty_prop.py:296-465, as mpmath numbers in numpy object arrays."""
    import mpmath as mp
    X, lam, sf = pb["X"], pb["lambdas"], pb["sigma_f"]
    N, D = X.shape
    ds = pb["ds"]
    with mp.workdps(dps):
        f = lambda x: mp.mpf(float(x))       # noqa: E731
        Xm = mp.matrix(N, D)
        for i in range(N):
            for k in range(D):
                Xm[i, k] = f(X[i, k])
        bm = [[f(beta[a][i]) for i in range(N)] for a in range(ds)]
        Wm = [[[f(W[a][j][i]) for j in range(N)] for i in range(N)] for a in range(ds)]          # [a][i][j], i <= j

        def step(um, Sm):
            mean, l = [None] * ds, [[None] * N for _ in range(ds)]
            cov = [[None] * ds for _ in range(ds)]
            v = [mp.matrix([um[k] - Xm[i, k] for k in range(D)]) for i in range(N)]
            for a in range(ds):
                La = mp.diag([f(x) for x in lam[a]])
                Li = mp.diag([1 / f(x) for x in lam[a]])
                B = mp.inverse(Sm + La)
                cm = f(sf[a]) ** 2 / mp.sqrt(mp.det(Li * Sm + mp.eye(D)))
                for i in range(N):
                    l[a][i] = cm * mp.exp(-(v[i].T * B * v[i])[0] / 2)
                mean[a] = mp.fsum(bm[a][i] * l[a][i] for i in range(N))
                A = mp.inverse(La / 2 + Sm)
                c = 1 / mp.sqrt(mp.det(2 * Li * Sm + mp.eye(D)))
                T = mp.mpf(0)
                for i in range(N):
                    for j in range(i, N):
                        s = v[i] + v[j]
                        T += Wm[a][i][j] * mp.exp(-(s.T * A * s)[0] / 8)
                cov[a][a] = f(sf[a]) ** 2 - c * T - mean[a] ** 2
            for a in range(ds):
                for b in range(ds):
                    if a == b:
                        continue
                    Lia, Lib = mp.diag([1 / f(x) for x in lam[a]]), mp.diag([1 / f(x) for x in lam[b]])
                    R = Sm * (Lia + Lib) + mp.eye(D)
                    Am = mp.inverse(R) * Sm
                    Kc = (f(sf[a]) * f(sf[b])) ** 2 / mp.sqrt(mp.det(R))
                    tot = mp.mpf(0)
                    for i in range(N):
                        for j in range(N):
                            di, dj = -v[i], -v[j]
                            z1, z2 = Lia * di, Lib * dj
                            if bug:     # :446 -- the quadratic terms as before, the cross term z2_i^T Am z1_j
                                cr = ((Lib * di).T * Am * (Lia * dj))[0]
                            else:
                                cr = (z1.T * Am * z2)[0]
                            ex = (-(di.T * Lia * di)[0] / 2 - (dj.T * Lib * dj)[0] / 2 + (z1.T * Am * z1)[0] / 2 + (z2.T * Am * z2)[0] / 2 + cr)
                            tot += bm[a][i] * bm[b][j] * mp.exp(ex)
                    cov[a][b] = Kc * tot - mean[a] * mean[b]
            return mean, cov, l

        um = [f(x) for x in u]
        Sm = mp.matrix(D, D)
        for k in range(D):
            for m in range(D):
                Sm[k, m] = (f(S[k][m]) + f(S[m][k])) / 2
        mean, cov, l = step(um, Sm)
        h = mp.mpf(10) ** (-dps // 3)
        out = {"mean": np.array(mean, dtype=object), "cov": np.array(cov, dtype=object), "l": np.array(l, dtype=object),
               "dmean_du": np.empty((ds, D), dtype=object), "dmean_dS": np.empty((ds, D, D), dtype=object),
               "dcov_du": np.empty((ds, ds, D), dtype=object), "dcov_dS": np.empty((ds, ds, D, D), dtype=object)}

        def diff(up, Sp, un, Sn):
            mp_, cp_, _ = step(up, Sp)
            mn_, cn_, _ = step(un, Sn)
            return ([(mp_[a] - mn_[a]) / (2 * h) for a in range(ds)],
                    [[(cp_[a][b] - cn_[a][b]) / (2 * h) for b in range(ds)] for a in range(ds)])
        for k in range(D):
            up, un = list(um), list(um)
            up[k] += h
            un[k] -= h
            dm, dc = diff(up, Sm, un, Sm)
            for a in range(ds):
                out["dmean_du"][a, k] = dm[a]
                for b in range(ds):
                    out["dcov_du"][a, b, k] = dc[a][b]
        for k in range(D):
            for m in range(k, D):
                Sp, Sn = Sm.copy(), Sm.copy()
                e = h if k == m else h / 2
                Sp[k, m] += e
                Sn[k, m] -= e
                if k != m:
                    Sp[m, k] += e
                    Sn[m, k] -= e
                dm, dc = diff(um, Sp, um, Sn)
                for a in range(ds):
                    out["dmean_dS"][a, k, m] = out["dmean_dS"][a, m, k] = dm[a]
                    for b in range(ds):
                        out["dcov_dS"][a, b, k, m] = out["dcov_dS"][a, b, m, k] = dc[a][b]
        return out
