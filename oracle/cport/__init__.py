"""TEST INFRASTRUCTURE ONLY: ctypes wrapper of the plain-C / OpenMP CPU port (oracle/cport/gpmpc_cpu.c)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        alt = os.environ.get("GPMPC_CPORT_LIB")           # the sanitizer build (make -C oracle/cport asan), tools/run_sanitizers.sh
        if alt:
            _LIB = ctypes.CDLL(alt)
            _LIB.gpmpc_cpu_rollout.restype = ctypes.c_int
            _LIB.gpmpc_cpu_rollout_fullcov.restype = ctypes.c_int
            return _LIB
        so = os.path.join(_HERE, "libgpmpc_cpu.so")
        srcs = [os.path.join(_HERE, f) for f in ("gpmpc_cpu.c", "gpmpc_cpu_fullcov.c", "gpmpc_cpu_ld.c", "gpmpc_cpu_given.c")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs):
            subprocess.run(["make", "-C", _HERE], check=True, capture_output=True)
        _LIB = ctypes.CDLL(so)
        _LIB.gpmpc_cpu_rollout.restype = ctypes.c_int
        _LIB.gpmpc_cpu_rollout_fullcov.restype = ctypes.c_int
    return _LIB


def rollout(pb, Ky_inv, gamma, x0=None, U=None, nthreads=0):
    """pb: dict from synth_problem; Ky_inv: (ds, N, N).  Returns dict(means, vars, cost, grad) as numpy arrays."""
    c = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64))      # noqa: E731
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))          # noqa: E731
    X, Y, lam, sf = c(pb["X"]), c(pb["Y"]), c(pb["lambdas"]), c(pb["sigma_f"])
    x0 = c(pb["x0"] if x0 is None else x0).reshape(-1, pb["ds"])
    U = c(pb["U"] if U is None else U)
    U = U.reshape(-1, U.shape[-2], pb["da"])
    B, H = U.shape[0], U.shape[1]
    K, Q, R, xr, ur = c(Ky_inv), c(pb["Q"]), c(pb["R"]), c(pb["x_ref"]), c(pb["u_ref"])
    means = np.zeros((B, H + 1, pb["ds"])); vars_ = np.zeros((B, H + 1, pb["ds"]))
    cost = np.zeros(B); grad = np.zeros((B, H, pb["da"]))
    rc = lib().gpmpc_cpu_rollout(X.shape[0], pb["ds"], pb["da"], H, B, p(X), p(K), p(Y), p(lam), p(sf), p(x0), p(U),
                                 ctypes.c_double(gamma), p(Q), p(R), p(xr), p(ur), p(means), p(vars_), p(cost), p(grad),
                                 int(nthreads))
    if rc != 0:
        raise RuntimeError(f"gpmpc_cpu_rollout failed: {rc}")
    return {"means": means, "vars": vars_, "cost": cost, "grad": grad}


def rollout_extended(pb, Ky_inv, x0=None, U=None, nthreads=0):
    """Forward pass (means, vars) of the diagonal rollout with every operation in x87 extended precision
    (oracle/cport/gpmpc_cpu_ld.c): the yardstick for the noise-level accuracy sweep.  Small N only."""
    c = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64))      # noqa: E731
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))          # noqa: E731
    X, Y, lam, sf = c(pb["X"]), c(pb["Y"]), c(pb["lambdas"]), c(pb["sigma_f"])
    x0 = c(pb["x0"] if x0 is None else x0).reshape(-1, pb["ds"])
    U = c(pb["U"] if U is None else U)
    U = U.reshape(-1, U.shape[-2], pb["da"])
    B, H = U.shape[0], U.shape[1]
    K = c(Ky_inv)
    means = np.zeros((B, H + 1, pb["ds"])); vars_ = np.zeros((B, H + 1, pb["ds"]))
    lib().gpmpc_cpu_rollout_ld.restype = ctypes.c_int
    rc = lib().gpmpc_cpu_rollout_ld(X.shape[0], pb["ds"], pb["da"], H, B, p(X), p(K), p(Y), p(lam), p(sf), p(x0), p(U),
                                    p(means), p(vars_), int(nthreads))
    if rc != 0:
        raise RuntimeError(f"gpmpc_cpu_rollout_ld failed: {rc}")
    return {"means": means, "vars": vars_}


def rollout_fullcov(pb, Ky_inv, gamma, x0=None, U=None, dirs=None, nthreads=0):
    """FULL-covariance rollout (oracle/cport/gpmpc_cpu_fullcov.c; BASELINE config 5).  dirs: optional (B, ndir, H, da)
    directions; ``ddir[b, d]`` is then the directional derivative dirs[b, d] . dcost_b/dU by the complex step.
    Returns dict(means (B,H+1,ds), covs (B,H+1,ds,ds), cost (B,), ddir (B,ndir))."""
    c = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64))      # noqa: E731
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))          # noqa: E731
    ds, da = pb["ds"], pb["da"]
    X, Y, lam, sf = c(pb["X"]), c(pb["Y"]), c(pb["lambdas"]), c(pb["sigma_f"])
    x0 = c(pb["x0"] if x0 is None else x0).reshape(-1, ds)
    U = c(pb["U"] if U is None else U)
    U = U.reshape(-1, U.shape[-2], da)
    B, H = U.shape[0], U.shape[1]
    K, Q, R, xr, ur = c(Ky_inv), c(pb["Q"]), c(pb["R"]), c(pb["x_ref"]), c(pb["u_ref"])
    dirs = np.zeros((B, 0, H, da)) if dirs is None else c(dirs).reshape(B, -1, H, da)
    ndir = dirs.shape[1]
    means = np.zeros((B, H + 1, ds)); covs = np.zeros((B, H + 1, ds, ds))
    cost = np.zeros(B); ddir = np.zeros((B, max(ndir, 1)))
    rc = lib().gpmpc_cpu_rollout_fullcov(X.shape[0], ds, da, H, B, p(X), p(K), p(Y), p(lam), p(sf), p(x0), p(U),
                                         ctypes.c_double(gamma), p(Q), p(R), p(xr), p(ur), p(means), p(covs), p(cost),
                                         ndir, p(dirs if ndir else np.zeros(1)), p(ddir), int(nthreads))
    if rc != 0:
        raise RuntimeError(f"gpmpc_cpu_rollout_fullcov failed: {rc}")
    return {"means": means, "covs": covs, "cost": cost, "ddir": ddir[:, :ndir]}


def moment_match_fullcov(X, Ky_inv, Y, lambdas, sigma_f, u, S, nthreads=0):
    """One moment-matching step for N(u, S) with a FULL covariance S: (mean (ds,), cov (ds, ds)) of the ds GP outputs
    (variances on the diagonal, consistent-form cross-covariances off it).  Y: (N, ds)."""
    c = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64))      # noqa: E731
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))          # noqa: E731
    X, K, Y, lam, sf, u, S = c(X), c(Ky_inv), c(Y), c(lambdas), c(sigma_f), c(u), c(S)
    N, D = X.shape
    ds = Y.shape[1]
    lib().gpmpc_cpu_moment_match_fullcov.restype = ctypes.c_int
    mean = np.zeros(ds); cov = np.zeros((ds, ds))
    rc = lib().gpmpc_cpu_moment_match_fullcov(N, ds, D, p(X), p(K), p(Y), p(lam), p(sf), p(u), p(S), p(mean), p(cov), int(nthreads))
    if rc != 0:
        raise RuntimeError(f"gpmpc_cpu_moment_match_fullcov failed: {rc}")
    return mean, cov


# ------------------------------------------------------------------------------------------------------------------------------
# oracle/cport/gpmpc_cpu_given.c: one step and the whole rollout on GIVEN constants, in double ("d") and long double ("ld")
# ------------------------------------------------------------------------------------------------------------------------------
_dbl = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64))          # noqa: E731
_dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))               # noqa: E731


def constants(pb, Ky_inv):
    """(beta (ds, N), W (ds, N, N)) by their numpy definitions (tests/test_gpu_parity.py::test_pack_constants), in the layout of
    ``GPPack.beta()`` / ``GPPack.weights()``: the pair (i <= j) at W[a, j, i], off-diagonal pairs doubled, zeros elsewhere."""
    X, Y, lam, sf, K = _dbl(pb["X"]), _dbl(pb["Y"]), _dbl(pb["lambdas"]), _dbl(pb["sigma_f"]), _dbl(Ky_inv)
    N, ds = X.shape[0], Y.shape[1]
    beta, W = np.zeros((ds, N)), np.zeros((ds, N, N))
    for a in range(ds):
        beta[a] = K[a] @ Y[:, a]
        d2 = np.zeros((N, N))
        for k in range(X.shape[1]):                           # (dimension by dimension: no N x N x D temporary at N = 2310)
            d2 += (X[:, None, k] - X[None, :, k]) ** 2 / lam[a, k]
        M = (0.5 * (K[a] + K[a].T) - np.outer(beta[a], beta[a])) * np.exp(-0.25 * d2) * sf[a] ** 4
        W[a] = (np.triu(M, 1) * 2 + np.diag(np.diag(M))).T
    return beta, W


def constants_ld(pb, Ky_inv):
    """The same constants with every operation in long double, as gpmpc_cpu_ld.c builds them: numpy ``longdouble`` arrays."""
    X, Y, lam, sf, K = _dbl(pb["X"]), _dbl(pb["Y"]), _dbl(pb["lambdas"]), _dbl(pb["sigma_f"]), _dbl(Ky_inv)
    N, ds = X.shape[0], Y.shape[1]
    assert np.dtype(np.longdouble).itemsize == 16 and np.finfo(np.longdouble).nmant == 63, "x87 extended precision expected"
    beta, W = np.zeros((ds, N), dtype=np.longdouble), np.zeros((ds, N, N), dtype=np.longdouble)
    f = lib().gpmpc_given_constants_ld
    f.restype = ctypes.c_int
    rc = f(N, ds, X.shape[1], _dp(X), _dp(K), _dp(Y), _dp(lam), _dp(sf), ctypes.c_void_p(beta.ctypes.data), ctypes.c_void_p(W.ctypes.data))
    if rc != 0:
        raise RuntimeError(f"gpmpc_given_constants_ld failed: {rc}")
    return beta, W


def _given_args(pb, beta, W):
    """The leading arguments every gpmpc_given_* entry takes; the arrays are returned too, to keep them alive over the call."""
    X, lam, sf = _dbl(pb["X"]), _dbl(pb["lambdas"]), _dbl(pb["sigma_f"])
    N, ds = X.shape[0], pb["ds"]
    cld = int(np.asarray(W).dtype == np.longdouble)
    dt = np.longdouble if cld else np.float64
    assert np.asarray(beta).dtype == dt
    beta = np.ascontiguousarray(np.asarray(beta)[:, :N], dtype=dt)
    W = np.ascontiguousarray(W, dtype=dt)
    Np = W.shape[-1]
    assert beta.shape == (ds, N) and W.shape == (ds, Np, Np) and Np >= N
    return (N, Np, ds), (_dp(X), _dp(lam), _dp(sf), ctypes.c_void_p(beta.ctypes.data), ctypes.c_void_p(W.ctypes.data), cld), (X, lam, sf, beta, W)


def _given_fn(name, prec):
    assert prec in ("d", "ld", "cd", "cld")
    f = getattr(lib(), "%s_%s" % (name, prec))
    f.restype = ctypes.c_int
    return f


def given_step_diag(pb, beta, W, u, s, prec="ld", nthreads=0):
    """nq diagonal moment-matching steps on given constants: u, s (nq, D) -> dict(mean, var, A_mean, A_var, A_exp), each (nq, ds)."""
    (N, Np, ds), cargs, keep = _given_args(pb, beta, W)
    D = pb["ds"] + pb["da"]
    u, s = _dbl(u).reshape(-1, D), _dbl(s).reshape(-1, D)
    nq = u.shape[0]
    out = [np.zeros((nq, ds)) for _ in range(5)]
    rc = _given_fn("gpmpc_given_step_diag", prec)(N, Np, ds, D, *cargs, nq, _dp(u), _dp(s), *[_dp(o) for o in out], int(nthreads))
    if rc != 0:
        raise RuntimeError(f"gpmpc_given_step_diag failed: {rc}")
    return dict(zip(("mean", "var", "A_mean", "A_var", "A_exp"), out))


def given_step_full(pb, beta, W, u, S, prec="ld", nthreads=0, bug=False, want_l=False):
    """nq full-covariance steps on given constants: u (nq, D), S (nq, D, D) -> dict(mean, A_mean (nq, ds), cov, A_cov (nq, ds, ds)).
    S is read as given (the HIP kernels read (S + S^T)/2: pass that).  bug: the reference's transposed cross term (GPMPC_COV_BUG_COMPAT),
    every ordered pair (a, b) a sum of its own.  want_l: also ``l`` (nq, ds, N), l_i = c_m exp(-1/2 v_i^T B v_i)."""
    (N, Np, ds), cargs, keep = _given_args(pb, beta, W)
    D = pb["ds"] + pb["da"]
    u, S = _dbl(u).reshape(-1, D), _dbl(S).reshape(-1, D, D)
    nq = u.shape[0]
    mean, A_mean, cov, A_cov = np.zeros((nq, ds)), np.zeros((nq, ds)), np.zeros((nq, ds, ds)), np.zeros((nq, ds, ds))
    l = np.zeros((nq, ds, N)) if want_l else None
    rc = _given_fn("gpmpc_given_step_full", prec)(N, Np, ds, D, *cargs, nq, _dp(u), _dp(S), _dp(mean), _dp(cov), _dp(A_mean), _dp(A_cov), int(nthreads),
                                                  int(bool(bug)), None if l is None else _dp(l))
    if rc != 0:
        raise RuntimeError(f"gpmpc_given_step_full failed: {rc}")
    out = {"mean": mean, "cov": cov, "A_mean": A_mean, "A_cov": A_cov}
    if want_l:
        out["l"] = l
    return out


def given_step_full_jac(pb, beta, W, u, S, prec="cld", nthreads=0, bug=False):
    """Jacobians of nq full-covariance steps by the complex step, at (S + S^T)/2 and symmetrised in S: dict(dmean_du (nq, ds, D),
    dmean_dS (nq, ds, D, D), dcov_du (nq, ds, ds, D), dcov_dS (nq, ds, ds, D, D)); the diagonal of dcov is the variance Jacobian.
    prec "cd" | "cld".  D + D (D + 1) / 2 runs of the step per query."""
    assert prec in ("cd", "cld")
    (N, Np, ds), cargs, keep = _given_args(pb, beta, W)
    D = pb["ds"] + pb["da"]
    u, S = _dbl(u).reshape(-1, D), _dbl(S).reshape(-1, D, D)
    nq = u.shape[0]
    out = {"dmean_du": np.zeros((nq, ds, D)), "dmean_dS": np.zeros((nq, ds, D, D)),
           "dcov_du": np.zeros((nq, ds, ds, D)), "dcov_dS": np.zeros((nq, ds, ds, D, D))}
    rc = _given_fn("gpmpc_given_step_full_jac", prec)(N, Np, ds, D, *cargs, nq, _dp(u), _dp(S), int(bool(bug)), _dp(out["dmean_du"]),
                                                      _dp(out["dmean_dS"]), _dp(out["dcov_du"]), _dp(out["dcov_dS"]), int(nthreads))
    if rc != 0:
        raise RuntimeError(f"gpmpc_given_step_full_jac failed: {rc}")
    return out


def given_rollout(pb, beta, W, gamma, x0=None, U=None, full=False, prec="ld", nthreads=0, init_cov=None, action_var=None, process_var=None):
    """Whole trajectories on given constants with the cost of src/mpc.py:179-198.  prec "d" / "ld": dict(means, vars or covs, cost);
    prec "cd" / "cld": dict(cost, grad), the gradient by the complex step, one run per entry of U (small H da only).
    init_cov (ds, ds), action_var (da,), process_var (ds,): the noise model of the pack, each None = the reference's constants."""
    (N, Np, ds), cargs, keep = _given_args(pb, beta, W)
    da = pb["da"]
    x0 = _dbl(pb["x0"] if x0 is None else x0).reshape(-1, ds)
    U = _dbl(pb["U"] if U is None else U)
    U = U.reshape(-1, U.shape[-2], da)
    B, H = U.shape[0], U.shape[1]
    Q, R, xr, ur = _dbl(pb["Q"]), _dbl(pb["R"]), _dbl(pb["x_ref"]), _dbl(pb["u_ref"])
    means, covs = np.zeros((B, H + 1, ds)), np.zeros((B, H + 1, ds, ds) if full else (B, H + 1, ds))
    cost, grad = np.zeros(B), np.zeros((B, H, da))
    noise = [None if a is None else _dbl(a).reshape(shape) for a, shape in ((init_cov, (ds, ds)), (action_var, (da,)), (process_var, (ds,)))]
    rc = _given_fn("gpmpc_given_rollout", prec)(int(bool(full)), N, Np, ds, da, H, B, *cargs, _dp(x0), _dp(U), ctypes.c_double(gamma), _dp(Q), _dp(R),
                                                _dp(xr), _dp(ur), _dp(means), _dp(covs), _dp(cost), _dp(grad), int(nthreads),
                                                *[None if a is None else _dp(a) for a in noise])
    if rc != 0:
        raise RuntimeError(f"gpmpc_given_rollout failed: {rc}")
    if prec in ("cd", "cld"):
        return {"cost": cost, "grad": grad}
    return {"means": means, "covs" if full else "vars": covs, "cost": cost}
