"""Extended-precision restatement of the PACK BUILD (csrc/pack_build.hip: k_pack_beta, k_pack_residual, k_pack_weights), the link between the
training data and the constants every rollout kernel reads.  TEST INFRASTRUCTURE ONLY.

Plain numpy in the working precision of tests/gpstate_reference.py (``np.longdouble``, object arrays of ``mpmath.mpf`` on request or where
the host has no extended type, ``prec=np.float64`` for the "honest float64 implementation" K_ref is measured on).  The functions take
what the kernels take: the float64 Ky_inv is data -- possibly NON-symmetric, one matrix per GP (ds, N, N) or one shared by all (N, N).

    beta[a][i]   = sum_j Kinv_a[i][j] y_a[j]                       (ROW form: K y, not K^T y)        unit A_beta = sum_j |Kinv_a[i][j] y_a[j]|
    r_a[j]       = y_a[j] - sum_k X[j][k] W[a][k] - c[a]           (nominal model)                   rho_a[j] = |y| + sum_k |X W| + |c|
    beta[a][i]   = sum_j Kinv_a[i][j] r_a[j]                                                         unit = sum_j |Kinv_a[i][j]| rho_a[j]
    M_a(i, j)    = w_ij (1/2 (K_ij + K_ji) - beta_i beta_j) sf_a^4 exp(-e_ij),   i <= j,   e_ij = 1/4 sum_k (x_ik - x_jk)^2 / lambda_ak,
                   w = 1 on the diagonal, 2 above it; beta is GIVEN (the float64 beta the pack exported), so the two links are judged apart
    A_M(i, j)    = w sf^4 exp(-e) [ |1/2 (K_ij + K_ji)| + |beta_i beta_j| + |1/2 (K_ij + K_ji) - beta_i beta_j| (1 + e) ]

The first two terms of A_M cover the cancelling difference, the (1 + e) term the roundings of the product and of the exponent as it passes
through exp.  K = |value - reference| / (2^-53 A): a unit free of the conditioning of the problem."""
import functools

import numpy as np

import gpstate_reference as R

U53 = 2.0 ** -53
ASYM = 1e-3
EXCESS_FACTOR = 10.0                                        # K <= 10 K_ref of the same case (the rule of tests/test_gpu_accuracy.py)
# Absolute caps per unit: twice the worst K measured on an MI355X over every case and entry point of tests/test_gpu_pack.py (its docstring
# states the measurements: beta 2.14, nominal beta 2.10, M 2.87), rounded up to two digits
CAP_K = {"beta": 4.3, "nominal": 4.2, "M": 5.8}
SIGMA_F_RANGE = (0.6, 1.8)                                  # tests/offgrid_problems.py draws its amplitudes from the same interval

# One point either side of every edge of the build kernels -- the 32 x 32 tiles of k_pack_weights (and its early-out for tiles below the
# diagonal), the padding of N to a multiple of 64, the four waves = four rows of a 256-thread block of k_pack_beta and its 64-lane stride,
# the 256-thread blocks of k_pack_points / k_pack_residual -- and a second block of each.
LADDER_N = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 255, 256, 257, 300, 520)
SHARED_AT = (31, 127, 129, 256)                             # cases whose GPs have bit-identical lambdas


def ladder():
    """[(N, D, ds, shared)]: D cycles through 1 ... 8; ds = D on the first pass (action_dim = 0, ds = 8 at N = 64), ceil(D / 2) on the
    second, 1 on the third (ds = 1: no GP pair)."""
    out = []
    for i, n in enumerate(LADDER_N):
        D = i % 8 + 1
        ds = max(1, D - (i // 8) * (D // 2))
        out.append((n, D, ds, n in SHARED_AT and ds >= 2))
    return out


def case_id(case):
    return "N%d-D%d-ds%d%s" % (case[0], case[1], case[2], "-shared" if case[3] else "")


def seed_of(n, D, ds):
    return 100000 * ds + R.seed_of(n, D)


def _inverse(X, lam, sf, noise, G):
    _, Ky = (R.to_f64(a) for a in R.build(X, lam, sf, noise))
    return np.linalg.inv(Ky + ASYM * (G - G.T))


def problem(n, D, ds, shared=False, one_matrix=False, spread=None):
    """ds GPs on the inputs X of ``gpstate_reference.problem`` (same seed rule), float64: lambda_a ~ U(0.7, 2.5) per GP (GP 0's for all when
    ``shared``), sigma_f,a ~ U(0.6, 1.8), targets Y (N, ds), and Kinv_a = inv(Ky_a + asym (G_a - G_a^T)), asym = 1e-3: genuinely
    NON-symmetric inverses (``one_matrix``: GP 0's matrix alone, shape (N, N), for the builds that share one).  Also a nominal model
    (W (ds, D), c (ds,)).  ``spread``: the second half of the points moved by that much along the first input, so that every weight
    between the halves underflows.  Read-only arrays, shared between tests: one dict per problem."""
    return _problem(n, D, ds, bool(shared), bool(one_matrix), spread)


@functools.lru_cache(maxsize=None)
def _problem(n, D, ds, shared, one_matrix, spread):
    seed = seed_of(n, D, ds)
    base = R.problem(seed, n, D, asym=ASYM)
    rng = np.random.default_rng(seed + 1)
    X = np.array(base["X"])
    if spread is not None:
        X[n // 2:, 0] += spread
    lam = rng.uniform(0.7, 2.5, (ds, D))
    if shared:
        lam[:] = lam[0]
    sf = rng.uniform(SIGMA_F_RANGE[0], SIGMA_F_RANGE[1], ds)
    Y = np.stack([(0.5 + 0.3 * a) * np.sin(X + 0.4 * a).sum(axis=1) for a in range(ds)], axis=1) + 0.1 * rng.standard_normal((n, ds))
    Kinv = np.stack([_inverse(X, lam[a], sf[a], base["noise"], rng.standard_normal((n, n))) for a in range(1 if one_matrix else ds)])
    out = {"n": n, "D": D, "ds": ds, "da": D - ds, "X": X, "Y": Y, "lam": lam, "sf": sf, "noise": base["noise"],
           "Kinv": Kinv[0] if one_matrix else Kinv, "W": rng.uniform(-0.6, 0.6, (ds, D)), "c": rng.uniform(-0.3, 0.3, ds)}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _matrix(Kinv, a):
    return Kinv if Kinv.ndim == 2 else Kinv[a]


def beta(Kinv, Y, prec=None):
    """(beta (ds, N), A_beta (ds, N)) from targets Y (N, ds): the row form K y."""
    Kinv, Y = R.cast(Kinv, prec), R.cast(Y, prec)
    val, mag = zip(*(R.dot_abs(_matrix(Kinv, a), Y[:, a]) for a in range(Y.shape[1])))
    return np.stack(val), np.stack(mag)


def residual(X, Y, W, c, prec=None):
    """(r (N, ds), rho (N, ds)): targets minus the nominal model, and the sum of the absolute values of the terms of each."""
    X, Y, W, c = R.cast(X, prec), R.cast(Y, prec), R.cast(W, prec), R.cast(c, prec)
    r, rho = Y - c[None, :], R._abs(Y) + R._abs(c)[None, :]
    for k in range(X.shape[1]):
        t = X[:, k][:, None] * W[:, k][None, :]
        r, rho = r - t, rho + R._abs(t)
    return r, rho


def beta_nominal(Kinv, X, Y, W, c, prec=None):
    """(beta (ds, N), unit (ds, N)) of a pack with the nominal model (W, c): Kinv r, in units of sum_j |Kinv_ij| rho_j."""
    r, rho = residual(X, Y, W, c, prec)
    Kinv = R.cast(Kinv, prec)
    ds = r.shape[1]
    return (np.stack([_matrix(Kinv, a) @ r[:, a] for a in range(ds)]),
            np.stack([R._abs(_matrix(Kinv, a)) @ rho[:, a] for a in range(ds)]))


def exponent(X, lam_a, prec=None):
    """e_ij = 1/4 sum_k (x_ik - x_jk)^2 / lambda_k, all pairs."""
    X, lam_a = R.cast(X, prec), R.cast(lam_a, prec)
    e = X[:, :1] * 0 + X[:, :1].T * 0
    for k in range(X.shape[1]):
        d = X[:, k][:, None] - X[:, k][None, :]
        e = e + d * d / lam_a[k]
    return e / 4


def weights(X, Kinv, beta_given, lam, sf, prec=None, exponent_map=None):
    """(M (ds, N, N), A_M (ds, N, N)), element (i, j) at [a, i, j] for i <= j and 0 below the diagonal; ``beta_given`` (ds, N) is data.
    ``exponent_map``: applied to e before exp (tests/test_host_pack.py emulates a rounded exponent with it)."""
    Kinv, b, sf = R.cast(Kinv, prec), R.cast(beta_given, prec), R.cast(sf, prec)
    n = len(X)
    upper = np.triu(np.ones((n, n), dtype=bool))
    w = np.triu(np.ones((n, n)), 1) + 1                                     # 1 on the diagonal, 2 above it (and below: masked)
    Ms, As = [], []
    for a in range(b.shape[0]):
        K = _matrix(Kinv, a)
        e = exponent(X, lam[a], prec)
        if exponent_map is not None:
            e = exponent_map(e)
        ksym = (K + K.T) / 2
        bb = np.outer(b[a], b[a])
        g = R.cast(w, prec) * (sf[a] * sf[a] * sf[a] * sf[a]) * R._exp(-e)
        M = (ksym - bb) * g
        A = g * (R._abs(ksym) + R._abs(bb) + R._abs(ksym - bb) * (1 + e))
        Ms.append(np.where(upper, M, M * 0))
        As.append(np.where(upper, A, A * 0))
    return np.stack(Ms), np.stack(As)


def k_of(got, ref, unit, mask=None):
    """max |got - ref| / (2^-53 unit) over the entries of ``mask`` (all by default); entries whose unit is 0 must agree exactly."""
    ref, unit = np.asarray(ref), np.asarray(unit)
    diff = np.abs(np.asarray(got).astype(ref.dtype) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(diff == 0, 0, diff / (U53 * unit))
    if mask is not None:
        k = k[mask]
    return float(k.max()) if k.size else 0.0


def budget(unit, kref):
    """What K of ``unit`` may reach on the case whose K_ref values are ``kref``: 10 K_ref and the absolute cap."""
    return min(EXCESS_FACTOR * kref[unit], CAP_K[unit])


def upper_mask(ds, n):
    return np.broadcast_to(np.triu(np.ones((n, n), dtype=bool)), (ds, n, n))


def k_ref(n, D, ds, shared=False, one_matrix=False, spread=None):
    """K_ref of a problem: the same formulas in plain float64 against the extended evaluation.  {"beta", "nominal", "M"} plus the
    conditioning of the inputs: "cancel" = max A_beta / |beta|, "emax" = the largest exponent."""
    return _k_ref(n, D, ds, bool(shared), bool(one_matrix), spread)


@functools.lru_cache(maxsize=None)
def _k_ref(n, D, ds, shared, one_matrix, spread):
    pr = problem(n, D, ds, shared, one_matrix, spread)
    b_ld, A_b = beta(pr["Kinv"], pr["Y"])
    b_64, _ = beta(pr["Kinv"], pr["Y"], np.float64)
    n_ld, A_n = beta_nominal(pr["Kinv"], pr["X"], pr["Y"], pr["W"], pr["c"])
    n_64, _ = beta_nominal(pr["Kinv"], pr["X"], pr["Y"], pr["W"], pr["c"], np.float64)
    M_ld, A_M = weights(pr["X"], pr["Kinv"], b_64, pr["lam"], pr["sf"])
    M_64, _ = weights(pr["X"], pr["Kinv"], b_64, pr["lam"], pr["sf"], np.float64)
    with np.errstate(divide="ignore"):
        cancel = float((A_b / np.abs(b_ld)).max())
    return {"beta": k_of(b_64, b_ld, A_b), "nominal": k_of(n_64, n_ld, A_n), "M": k_of(M_64, M_ld, A_M, upper_mask(ds, n)),
            "cancel": cancel, "emax": float(max(exponent(pr["X"], pr["lam"][a]).max() for a in range(ds)))}
