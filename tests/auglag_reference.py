"""numpy restatement of the augmented-Lagrangian rule of the constrained multi-start (include/gpmpc.h): merit, outer
step, finish and the solve loop over an ``evaluate(X) -> f (K,), grad (K, n), g (K, R), g_jac (K, R, n)`` callback, with
tests/lbfgs_reference.py as the inner search.

Written from the rule, sharing no code with csrc/auglag.hip.  A state is a dict of arrays over the K starts:
    rho, V_prev, v, f, inc_v, inc_f (K,); lam (K, R); inc_x (K, n); alive, settled (K,) bool.
Every function takes ``dtype``-agnostic arrays: a state of np.longdouble arrays is advanced in np.longdouble (the tolerance of the GPU parity
tests is measured that way).  ``outer`` also returns a report: for every inequality of the rule that compares computed quantities, the two
sides -- the parity test asserts that none of them is decided by rounding."""
import numpy as np

import lbfgs_reference as LR

DEFAULTS = dict(rho0=10.0, growth=10.0, shrink=0.25, rho_max=1e8, lam_max=1e12, feas_tol=1e-4)


def psi_of(g, lam, rho):
    t = lam + rho[:, None] * g
    with np.errstate(invalid="ignore"):
        return np.where(t > 0, t, np.where(t <= 0, np.zeros_like(t), t)), t            # (a NaN passes through)


def merit(f, grad, g, g_jac, lam, rho):
    """(M (K,), dM (K, n)): rows i ascending, one chain each; a row with psi_i == 0 is not read."""
    K, n = grad.shape
    R = g.shape[1]
    psi, _ = psi_of(g, lam, rho)
    s = np.zeros(K, dtype=grad.dtype)
    acc = np.zeros((K, n), dtype=grad.dtype)
    for i in range(R):
        s = s + (psi[:, i] * psi[:, i] - lam[:, i] * lam[:, i])
        on = psi[:, i] != 0
        acc[on] = acc[on] + psi[on, i][:, None] * g_jac[on, i, :]
    with np.errstate(invalid="ignore"):
        return f + (1.0 / (2.0 * rho)) * s, grad + acc


def new_state(X0c, R, rho0=10.0):
    """The state a solve starts from; X0c (K, n): the clipped start points."""
    K = X0c.shape[0]
    dt = X0c.dtype
    inf = lambda: np.full(K, np.inf, dtype=dt)               # noqa: E731
    return {"rho": np.full(K, rho0, dtype=dt), "V_prev": inf(), "v": inf(), "f": inf(), "inc_v": inf(), "inc_f": inf(),
            "lam": np.zeros((K, R), dtype=dt), "inc_x": X0c.copy(), "alive": np.ones(K, dtype=bool), "settled": np.zeros(K, dtype=bool)}


def outer(st, f, g, X, conv, update, growth=10.0, shrink=0.25, rho_max=1e8, lam_max=1e12, feas_tol=1e-4, want_report=False, **_):
    """One outer step from the evaluation (f, g) of the points X.  Returns the new state (the old one is not changed)."""
    st = {k: np.array(v, copy=True) for k, v in st.items()}
    dt = st["rho"].dtype
    f, g, X = np.asarray(f, dtype=dt), np.asarray(g, dtype=dt), np.asarray(X, dtype=dt)
    K = len(f)
    conv = np.zeros(K, dtype=bool) if conv is None else np.asarray(conv, dtype=bool)
    live = np.isfinite(f) & np.isfinite(g).all(axis=1)       # a dead start keeps everything
    rep = {"dead": ~live}
    i = np.where(live)[0]
    if len(i) == 0:
        return (st, rep) if want_report else st
    fi, gi = f[i], g[i]
    v = np.maximum(gi, 0).max(axis=1)
    kv = np.where(v <= feas_tol, np.zeros_like(v), v)
    iv, ic = st["inc_v"][i], st["inc_f"][i]
    better = (kv < iv) | ((kv == iv) & (fi < ic))
    rep["feasible"] = (i, v, feas_tol)
    rep["key"] = (i, kv, iv, fi, ic, better)
    b = i[better]
    st["inc_v"][b], st["inc_f"][b], st["inc_x"][b] = kv[better], fi[better], X[b]
    st["v"][i], st["f"][i] = v, fi
    if update:
        lam, rho = st["lam"][i], st["rho"][i]
        V = np.abs(np.maximum(gi, -lam / rho[:, None])).max(axis=1)
        t = lam + rho[:, None] * gi
        st["lam"][i] = np.minimum(lam_max, np.maximum(0, t))
        rep["lam"] = (i, t, lam_max)
        bound = shrink * st["V_prev"][i]
        grow = V > bound
        rep["grow"] = (i, V, bound, grow)
        grown = growth * rho
        rep["cap"] = (i[grow], grown[grow], rho_max)
        st["rho"][i] = np.where(grow, np.minimum(rho_max, grown), rho)
        st["V_prev"][i] = V
        st["settled"][i] = (V <= feas_tol) & conv[i]
        rep["settle"] = (i, V, feas_tol)
    return (st, rep) if want_report else st


def finish(st, alive=None):
    """(best, (inc_v, inc_f) of best, alive starts not settled): argmin of the keys, lowest index on ties."""
    if alive is not None:
        st["alive"] = np.asarray(alive, dtype=bool).copy()
    order = sorted(range(len(st["inc_v"])), key=lambda k: (st["inc_v"][k], st["inc_f"][k], k))
    best = order[0]
    return best, (st["inc_v"][best], st["inc_f"][best]), int((st["alive"] & ~st["settled"]).sum())


def solve(evaluate, X0, lb, ub, outer_iterations=8, inner_ticks=25, history=8, gtol=1e-6, ftol=1e-12, c1=1e-4, min_step=1e-12, trace=None,
          **rule):
    """The solve loop of the rule.  Returns (plan of the best incumbent, info); ``trace`` (a list) receives after every outer iteration a
    dict(o, state, inner) -- the state after the outer step, the inner state after the ticks."""
    rule = {**DEFAULTS, **rule}
    X0 = np.asarray(X0)
    K, n = X0.shape
    lb = np.broadcast_to(np.asarray(lb, dtype=X0.dtype), (n,))
    ub = np.broadcast_to(np.asarray(ub, dtype=X0.dtype), (n,))
    U = np.clip(X0, lb, ub)
    st, inner, evaluations = None, None, 0
    for o in range(outer_iterations):
        if o > 0:
            U = inner["X"].copy()
        f, grad, g, g_jac = evaluate(U)
        evaluations += 1
        if st is None:
            st = new_state(U, g.shape[1], rule["rho0"])
        st = outer(st, f, g, U, None if inner is None else inner["converged"], o > 0, **rule)
        M, dM = merit(f, grad, g, g_jac, st["lam"], st["rho"])
        inner = LR.start(U, M, dM, lb, ub, history, gtol)
        for _ in range(inner_ticks):
            if inner["done"].all():                          # (a done start ignores its evaluation: nothing left to advance)
                break
            f, grad, g, g_jac = evaluate(LR.trial_points(inner))
            evaluations += 1
            M, dM = merit(f, grad, g, g_jac, st["lam"], st["rho"])
            inner = LR.tick(inner, M, dM, lb, ub, gtol, ftol, c1, min_step)
        if trace is not None:
            trace.append({"o": o, "state": {k: np.array(v, copy=True) for k, v in st.items()}, "inner": inner})
    if inner is not None:
        U = inner["X"].copy()
    f, grad, g, g_jac = evaluate(U)
    evaluations += 1
    if st is None:
        st = new_state(U, g.shape[1], rule["rho0"])
    st = outer(st, f, g, U, None, False, **rule)
    best, key, open_ = finish(st, None if inner is None else inner["alive"])
    info = {"f": st["inc_f"], "violation": st["inc_v"], "feasible": st["inc_v"] == 0, "x": st["inc_x"], "best": best, "rho": st["rho"],
            "lam": st["lam"], "outer": outer_iterations, "evaluations": evaluations, "settled": st["settled"], "alive": st["alive"],
            "not_settled": open_, "state": st, "inner": inner}
    return st["inc_x"][best].copy(), info
