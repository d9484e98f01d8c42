"""numpy restatement of the lock-step multi-start L-BFGS rule (include/gpmpc.h) as functions state -> state.

Written from the rule, sharing no code with csrc/lbfgs.hip; tests/test_host_lbfgs.py pins it, iterated, to multistart.lockstep_lbfgs
(line_points = 1, no patience) bit for bit.  A state is a dict of arrays over the K starts:
    X, G, D, XT (K, n); F, A (K,); S, Y (K, m, n) and rho (K, m) NEWEST PAIR FIRST; cnt, iters (K,) int64; alive, done, converged (K,) bool.
Every function takes ``dtype``-agnostic arrays: a state of np.longdouble arrays is advanced in np.longdouble (the tolerance of the GPU parity
test is measured that way).  ``tick`` also returns a report: which branch every start took and, for every inequality of the rule that
compares computed quantities, the two sides -- the parity test asserts that none of them is decided by rounding."""
import numpy as np


def _dot(a, b):
    return np.einsum("kn,kn->k", a, b)


def _two_loop(g, S, Y, rho, cnt):
    """-H g per start, two-loop recursion over the stored pairs, newest first; pairs past cnt take no part."""
    m = min(S.shape[1], int(cnt.max())) if len(cnt) else 0
    q = g.copy()
    if m == 0:
        return -q
    alpha = []
    for j in range(m):
        a = np.where(j < cnt, rho[:, j] * _dot(S[:, j], q), 0.0)
        alpha.append(a)
        q -= a[:, None] * Y[:, j]
    yy = _dot(Y[:, 0], Y[:, 0])
    ok = (cnt > 0) & (yy > 0)
    q *= np.where(ok, 1.0 / np.where(ok, rho[:, 0] * yy, 1.0), 1.0)[:, None]
    for j in range(m - 1, -1, -1):
        b = np.where(j < cnt, rho[:, j] * _dot(Y[:, j], q), 0.0)
        q += np.where(j < cnt, alpha[j] - b, 0.0)[:, None] * S[:, j]
    return -q


def free_mask(x, g, lb, ub):
    return ~(((x <= lb) & (g > 0)) | ((x >= ub) & (g < 0)))


def _direction(st, lb, ub, report=None):
    """(D, a0, max |g_free|) of every start from its (X, G) and pairs; a start whose direction is no descent direction falls back to
    steepest descent and drops its pairs (st["cnt"] is changed in place)."""
    fm = free_mask(st["X"], st["G"], lb, ub)
    gf = np.where(fm, st["G"], 0.0)
    d = np.where(fm, _two_loop(gf, st["S"], st["Y"], st["rho"], st["cnt"]), 0.0)
    slope = _dot(d, gf)
    bad = ~(slope < 0) | ~np.isfinite(d).all(axis=1)
    if report is not None:
        report["slope"] = (slope.copy(), np.einsum("kn,kn->k", np.abs(d), np.abs(gf)))
        report["reset"] = bad & (st["cnt"] > 0)
    if bad.any():
        d[bad] = -gf[bad]
        st["cnt"][bad] = 0
    gn = np.sqrt(_dot(gf, gf))
    a0 = np.where(st["cnt"] == 0, np.minimum(1.0, 1.0 / np.where(gn > 0, gn, 1.0)), 1.0)
    return d, a0, np.abs(gf).max(axis=1)


def start(X0, F, G, lb, ub, history, gtol=1e-4):
    """The start step from the evaluation (F, G) of clip(X0)."""
    X = np.clip(np.asarray(X0), lb, ub)
    dt = X.dtype
    K, n = X.shape
    F, G = np.array(F, dtype=dt, copy=True).reshape(K), np.array(G, dtype=dt, copy=True).reshape(K, n)
    alive = np.isfinite(F) & np.isfinite(G).all(axis=1)
    m = history
    st = {"X": X, "F": np.where(alive, F, np.inf).astype(dt), "G": np.where(alive[:, None], G, 0.0).astype(dt),
          "S": np.zeros((K, m, n), dtype=dt), "Y": np.zeros((K, m, n), dtype=dt), "rho": np.zeros((K, m), dtype=dt),
          "cnt": np.zeros(K, dtype=np.int64), "iters": np.zeros(K, dtype=np.int64), "alive": alive, "done": ~alive}
    D, A, pg = _direction(st, lb, ub)
    st["D"], st["A"] = D, A.astype(dt)
    st["done"] = st["done"] | (pg <= gtol)
    st["converged"] = st["done"] & alive
    st["XT"] = np.clip(X + st["A"][:, None] * D, lb, ub)
    return st


def trial_points(st):
    """The batch a tick evaluates: XT, X for a done start."""
    return np.where(st["done"][:, None], st["X"], st["XT"])


def tick(st, ft, gt, lb, ub, gtol=1e-4, ftol=1e-10, c1=1e-4, min_step=1e-12, want_report=False):
    """One tick from the evaluation (ft, gt) of trial_points(st).  Returns the new state (the old one is not changed)."""
    st = {k: np.array(v, copy=True) for k, v in st.items()}
    X, F, G, D, A, XT, S, Y, rho, cnt = (st[k] for k in ("X", "F", "G", "D", "A", "XT", "S", "Y", "rho", "cnt"))
    K, n = X.shape
    m = S.shape[1]
    dt = X.dtype
    done, converged, iters = st["done"], st["converged"], st["iters"]
    ft, gt = np.asarray(ft, dtype=dt).reshape(K), np.asarray(gt, dtype=dt).reshape(K, n)
    rep = {"branch": np.array(["done" if d else "" for d in done], dtype=object)}
    step = XT - X
    finite = np.isfinite(ft) & np.isfinite(gt).all(axis=1)
    rhs = F + c1 * _dot(G, step)
    with np.errstate(invalid="ignore"):
        ok = finite & ~done & (ft <= rhs)
    rep["armijo"] = (np.where(finite & ~done, ft, np.nan), np.where(finite & ~done, rhs, np.nan))
    rep["nonfinite_f"], rep["nonfinite_g"] = ~np.isfinite(ft) & ~done, ~np.isfinite(gt).all(axis=1) & ~done
    shrink = ~ok & ~done
    if ok.any():
        i = np.where(ok)[0]
        s, y = step[i], gt[i] - G[i]
        sy = _dot(s, y)
        thr = 1e-10 * np.sqrt(_dot(s, s) * _dot(y, y))
        good = sy > thr
        rep["pair"] = (i, sy, thr, good)
        ig = i[good]
        S[ig, 1:], Y[ig, 1:], rho[ig, 1:] = S[ig, :-1], Y[ig, :-1], rho[ig, :-1]
        S[ig, 0], Y[ig, 0], rho[ig, 0] = s[good], y[good], 1.0 / sy[good]
        rep["wrapped"] = np.zeros(K, dtype=bool)
        rep["wrapped"][ig] = cnt[ig] == m
        cnt[ig] = np.minimum(cnt[ig] + 1, m)
        gain, bound = F[i] - ft[i], ftol * np.maximum(np.maximum(np.abs(F[i]), np.abs(ft[i])), 1.0)
        small = gain <= bound
        rep["small"] = (i, gain, bound)
        X[i], F[i], G[i] = XT[i], ft[i], gt[i]
        iters[i] += 1
        dr = {}
        Dn, An, pgn = _direction(st, lb, ub, dr)
        D[i], A[i] = Dn[i], An[i]
        rep["slope"] = (i, dr["slope"][0][i], dr["slope"][1][i])
        rep["reset"] = np.zeros(K, dtype=bool)
        rep["reset"][i] = dr["reset"][i]
        rep["pg"] = (i, pgn[i])
        fin = np.zeros(K, dtype=bool)
        fin[i] = small | (pgn[i] <= gtol)
        for k, g_, s_, p_ in zip(i, good, small, pgn[i]):
            rep["branch"][k] = "accept" + ("+pair" if g_ else "-pair") + ("+ftol" if s_ else "") + ("+gtol" if p_ <= gtol else "")
        converged |= fin
        done |= fin
    if shrink.any():
        A[shrink] *= 0.5
        reach = A * np.abs(D).max(axis=1)
        stalled = shrink & (reach < min_step)
        rep["stall"] = (np.where(shrink)[0], reach[shrink])
        for k in np.where(shrink)[0]:
            rep["branch"][k] = "stall" if stalled[k] else "shrink"
        converged |= stalled
        done |= stalled
    st["XT"] = np.clip(X + A[:, None] * D, lb, ub)
    return (st, rep) if want_report else st


def finish(st):
    """(best, F[best], starts not done)."""
    F = st["F"]
    best = int(np.argmin(F)) if np.isfinite(F).any() else 0
    return best, F[best], int((~st["done"]).sum())


def solve(evaluate, X0, lb, ub, max_ticks=300, history=8, gtol=1e-4, ftol=1e-10, c1=1e-4, min_step=1e-12, trace=None):
    """The rule iterated as multistart.lockstep_lbfgs iterates it; returns (x_best, info) with that function's keys.
    ``trace``: a list that receives every start's branch of every tick."""
    X0c = np.clip(np.asarray(X0, dtype=np.float64), lb, ub)
    n = X0c.shape[1]
    lb = np.broadcast_to(np.asarray(lb, dtype=np.float64), (n,))
    ub = np.broadcast_to(np.asarray(ub, dtype=np.float64), (n,))
    F, G = evaluate(X0c)
    st = start(X0c, F, G, lb, ub, history, gtol)
    ticks = 0
    while ticks < max_ticks and not st["done"].all():
        ft, gt = evaluate(trial_points(st))
        if trace is None:
            st = tick(st, ft, gt, lb, ub, gtol, ftol, c1, min_step)
        else:
            st, rep = tick(st, ft, gt, lb, ub, gtol, ftol, c1, min_step, want_report=True)
            trace.append(list(rep["branch"]))
        ticks += 1
    best = finish(st)[0]
    info = {"f": st["F"], "x": st["X"], "ticks": ticks, "evaluations": ticks + 1, "converged": st["converged"], "alive": st["alive"],
            "best": best, "iterations": st["iters"], "state": st}
    return st["X"][best].copy(), info
