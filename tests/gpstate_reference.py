"""Extended-precision restatement of the GP-state entry points (gpmpc_build_ky, gpmpc_predict, gpmpc_matvec, gpmpc_kinv_append,
gpmpc_gp_append, gpmpc_kinv_remove, gpmpc_gp_replace, gpmpc_ml_grad).  TEST INFRASTRUCTURE ONLY.

Plain numpy in ``np.longdouble`` (x87 extended: 64-bit mantissa, eps 1.08e-19) where the host has it, object arrays of ``mpmath.mpf``
otherwise (and on request: ``prec="mp"`` evaluates the same lines at the working precision of mpmath, which is how
tests/test_host_gpstate.py holds the block-inverse formulas to 1e-25).  ``prec=np.float64`` gives the "honest float64 implementation"
the GPU tolerances are sized against.

The functions take what the kernels take -- the float64 Ky_inv handed to a kernel is data, not something to re-derive -- and write
the definitions out with none of the kernels' groupings.  Every block-inverse formula is stated for a general NON-symmetric K
bordered by the same vector as row and column; row and column forms (K k / K^T k, K[:, p] / K[p, :], K* K / K* K^T) are distinct.
Dot products the GPU tests bound by ``tol * sum |terms|`` come back together with that sum."""
import numpy as np

LD = np.longdouble
HAVE_LD = np.finfo(LD).nmant >= 63
MP = "mp"
DEFAULT = LD if HAVE_LD else MP
MP_MIN_PREC = 80                      # bits, when mpmath stands in for a missing long double


def _mpmath():
    import mpmath
    return mpmath


def cast(a, prec=None):
    """`a` as an array of the working precision: longdouble / float64, or an object array of mpf."""
    prec = DEFAULT if prec is None else prec
    if prec is MP or prec == MP:
        mp = _mpmath()
        if isinstance(a, mp.mpf):
            return a
        a = np.asarray(a)
        if a.dtype == object:
            return a if a.ndim else a.item()
        return np.frompyfunc(lambda v: mp.mpf(float(v)), 1, 1)(a.astype(np.float64)) if a.ndim else mp.mpf(float(a))
    a = np.asarray(a, dtype=prec)
    return a if a.ndim else a[()]


def _exp(a):
    if a.dtype == object:
        return np.frompyfunc(_mpmath().exp, 1, 1)(a)
    return np.exp(a)


def _abs(a):
    return np.frompyfunc(abs, 1, 1)(a) if a.dtype == object else np.abs(a)


def to_f64(a):
    return np.asarray(a).astype(np.float64)


def kernel(A, B, lam, sf, prec=None):
    """k(a, b) = sf^2 exp(-1/2 sum_k (a_k - b_k)^2 / lambda_k), all pairs: (len(A), len(B))."""
    A, B, lam, sf = cast(A, prec), cast(B, prec), cast(lam, prec), cast(sf, prec)
    e = A[:, :1] * 0 + B[:, :1].T * 0                                   # zeros of the working precision
    for k in range(A.shape[1]):
        d = A[:, k][:, None] - B[:, k][None, :]
        e = e + d * d / lam[k]
    return sf * sf * _exp(-e / 2)


def build(X, lam, sf, noise, prec=None):
    """Kf = k(X, X), Ky = Kf + noise I."""
    Kf = kernel(X, X, lam, sf, prec)
    Ky = Kf.copy()
    noise = cast(noise, prec)
    for i in range(len(Ky)):
        Ky[i, i] = Ky[i, i] + noise
    return Kf, Ky


def dot_abs(A, B):
    """A @ B and |A| @ |B| (the sum of absolute terms of every dot product)."""
    return A @ B, _abs(A) @ _abs(B)


def predict(X, lam, sf, beta, Kinv, noise, Xp, prec=None):
    """Ks = k(Xp, X); mean = Ks beta; W = Ks Kinv (NOT Ks Kinv^T); cov[r][s] = k(xp_r, xp_s) - W[r] . Ks[s] + noise [r == s]."""
    Ks = kernel(Xp, X, lam, sf, prec)
    beta, Kinv, noise, sf = cast(beta, prec), cast(Kinv, prec), cast(noise, prec), cast(sf, prec)
    mean, mean_abs = dot_abs(Ks, beta)
    W, W_abs = dot_abs(Ks, Kinv)
    cov = kernel(Xp, Xp, lam, sf, prec) - W @ Ks.T
    for r in range(len(cov)):
        cov[r, r] = cov[r, r] + noise
    cov_abs = sf * sf + W_abs @ _abs(Ks).T                               # sf^2 + sum_i sum_k |Ks_rk| |Kinv_ki| |Ks_si|
    return {"Ks": Ks, "mean": mean, "mean_abs": mean_abs, "W": W, "W_abs": W_abs, "cov": cov, "cov_abs": cov_abs}


def append(Kinv, k, kappa, prec=None):
    """Inverse of [[K, k], [k^T, kappa]] from Kinv = K^-1:  v = Kinv k, w = Kinv^T k, q = 1 / (kappa - k . v),
    [[Kinv + q v w^T, -q v], [-q w^T, q]]."""
    Kinv, k, kappa = cast(Kinv, prec), cast(k, prec), cast(kappa, prec)
    n = len(k)
    v, w = Kinv @ k, Kinv.T @ k
    q = 1 / (kappa - k @ v)
    out = np.empty((n + 1, n + 1), dtype=Kinv.dtype)
    out[:n, :n] = Kinv + q * np.outer(v, w)
    out[:n, n] = -q * v
    out[n, :n] = -q * w
    out[n, n] = q
    return out


def remove(Kinv, p, prec=None):
    """Inverse of K without row and column p:  b = Kinv[:, p], c = Kinv[p, :], d = Kinv[p, p];  Kinv - b c^T / d, row / column p dropped."""
    Kinv = cast(Kinv, prec)
    b, c, d = Kinv[:, p], Kinv[p, :], Kinv[p, p]
    A = Kinv - np.outer(b, c) / d
    keep = [i for i in range(len(Kinv)) if i != p]
    return A[keep][:, keep]


def replace(Kinv, kt, kappa, p, prec=None):
    """Inverse of K with row and column p replaced by kt (entry p of kt is ignored) and kappa on the diagonal:
    v = Kinv kt - b (c . kt) / d,  w = Kinv^T kt - c (b . kt) / d,  q = 1 / (kappa - kt . v),
    out = Kinv - b c^T / d + q v w^T off row / column p;  out[:, p] = -q v;  out[p, :] = -q w;  out[p, p] = q."""
    Kinv, kt, kappa = cast(Kinv, prec), cast(kt, prec).copy(), cast(kappa, prec)
    kt[p] = kt[p] * 0
    b, c, d = Kinv[:, p], Kinv[p, :], Kinv[p, p]
    v = Kinv @ kt - b * ((c @ kt) / d)
    w = Kinv.T @ kt - c * ((b @ kt) / d)
    q = 1 / (kappa - kt @ v)
    out = Kinv - np.outer(b, c) / d + q * np.outer(v, w)
    out[:, p] = -q * v
    out[p, :] = -q * w
    out[p, p] = q
    return out


def ml_grad(X, Kinv, alpha, resid, lam, sf, noise, prec=None):
    """The D + 3 outputs of gpmpc_ml_grad from 1/2 tr((alpha alpha^T - Kinv) dKy/dtheta):
      dKy/dlog lambda_k = Kf o (x_ik - x_jk)^2 / (2 lambda_k),  dKy/dlog sigma_f = 2 Kf,  dKy/dlog sigma_n = 2 noise I,
    then r . alpha.  Returns (values, sums of absolute terms); the terms are alpha_i alpha_j dKy_ij / 2 and Kinv_ij dKy_ij / 2."""
    Kf = kernel(X, X, lam, sf, prec)
    X, Kinv, alpha, resid, lam, noise = (cast(a, prec) for a in (X, Kinv, alpha, resid, lam, noise))
    D = X.shape[1]
    aa = np.outer(alpha, alpha)
    M, Mabs = aa - Kinv, _abs(aa) + _abs(Kinv)
    val, mag = [], []
    for k in range(D):
        d = X[:, k][:, None] - X[:, k][None, :]
        dK = Kf * d * d / (2 * lam[k])
        val.append((M * dK).sum() / 2)
        mag.append((Mabs * dK).sum() / 2)
    val.append((M * Kf).sum())
    mag.append((Mabs * Kf).sum())
    val.append(noise * np.trace(M))
    mag.append(noise * np.trace(Mabs))
    val.append(resid @ alpha)
    mag.append(_abs(resid) @ _abs(alpha))
    return np.array(val, dtype=Kf.dtype), np.array(mag, dtype=Kf.dtype)


NP_MAX = 17                             # test points a problem carries (the GPU tests take the first p)


def problem(seed, n, D, sigma_n=0.3 * 1.2, asym=1e-3):
    """Test inputs, float64: X ~ U(-2, 2), lambda ~ U(0.7, 2.5), sigma_f = 1.2, Kf / Ky rounded from `build`, and
    Kinv = inv(Ky + E), E = asym (G - G^T), G standard normal: a genuinely non-symmetric inverse, so that exchanging a row form
    for a column form moves a result by percents, not by round-off.  Also a new input `xnew`, test points `Xp`, targets `y`,
    and beta = alpha = Kinv y as the library's callers form it (float64, data to the kernels)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (n, D))
    lam = rng.uniform(0.7, 2.5, D)
    sf, noise = 1.2, sigma_n ** 2
    G = rng.standard_normal((n, n))
    Kf, Ky = (to_f64(a) for a in build(X, lam, sf, noise))
    Kinv = np.linalg.inv(Ky + asym * (G - G.T))
    xnew = rng.uniform(-2, 2, D)
    Xp = rng.uniform(-2, 2, (NP_MAX, D))
    y = np.sin(X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    beta = Kinv @ y
    out = {"n": n, "D": D, "X": X, "lam": lam, "sf": sf, "noise": noise, "Kf": Kf, "Ky": Ky, "Kinv": Kinv, "xnew": xnew, "Xp": Xp,
           "y": y, "beta": beta}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)                                     # shared between tests: nobody modifies it
    return out


# The shape ladder of the GPU tests: one either side of every tile edge of the kernels (8-row groups of k_ml_partial / k_pred_w,
# 16 contraction slices and 64-column blocks of k_pred_w, 256-column blocks of the fills), a second block of each, and n = 1, 2.
LADDER_N = (1, 2, 7, 8, 9, 15, 17, 63, 64, 65, 255, 256, 257, 300, 520)


def ladder(schur=False):
    """[(n, D)]: D cycles through 1..8; for the Schur updates D >= 3 wherever n >= 255 (with D <= 2 and 257 points on [-2, 2]^D the
    condition of Ky passes 2e3 and an honest float64 evaluation no longer sits ten-fold under the GPU tolerance)."""
    out = []
    for i, n in enumerate(LADDER_N):
        D = i % 8 + 1
        if schur and n >= 255:
            D = max(D, 3)
        out.append((n, D))
    return out


def slots(n):
    """Slots removed / replaced at size n: both ends, the middle, and either side of the 256-column block edge."""
    return sorted({0, n // 2, n - 1} | {s for s in (255, 256) if s < n})


def seed_of(n, D):
    return 1000 * n + D
