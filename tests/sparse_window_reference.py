"""Extended-precision restatement of the sparse-GP window: gpmpc_sparse_remove, gpmpc_sparse_replace and a chain of replacements as
SparseGPState runs it.  TEST INFRASTRUCTURE ONLY; everything else comes from tests/sparse_reference.py (imported as ``R``).

``remove`` is the inverse of ``R.append`` written out plainly; ``replace`` is remove-then-append, the plain way (NOT the device's fused
route, which is ``replace_fused``: the same numbers by t_n = s_n + c t_o, kept apart so that it can serve as a held-out evaluation);
``chain`` fits the first ``window`` rows and replaces in ring order with the refresh and rebase counters of the state.

A removal cancels: den = Lambda - v . t reached 8e-3 Lambda on the ladder, and the float64 error then depends on the ORDER of the sums
far more than it does for an append.  ``prec=np.float64`` therefore exists in several summation orders of every dot product
(``order``): "numpy" (the ``@`` of numpy), "asc" and "desc" (sequential sums, ascending and descending index) and ("perm", seed) (a
sequential sum in a fixed permutation).  The allowance of a device output, ``allowance4``, takes the LARGEST error of the four
``ORDERS`` evaluations: max(8 e64_4orders, 1e-13 max|ref|); ``HELD_OUT`` are the evaluations that rule is checked against on the CPU
(tests/test_host_sparse_window.py)."""
import functools

import numpy as np

import sparse_reference as R
from sparse_reference import cast, kernel

ORDERS = ("numpy", "asc", "desc", ("perm", 0))
HELD_OUT = (("perm", 1), ("perm", 2), ("perm", 3))


def _index(n, order):
    if order == "asc":
        return range(n)
    if order == "desc":
        return range(n - 1, -1, -1)
    return np.random.default_rng(1000 + order[1]).permutation(n)


def _mv(A, x, order="numpy"):
    """A @ x (x a vector or a matrix) with every dot product summed in ``order``."""
    if order == "numpy":
        return A @ x
    acc = (A[:, :1] * 0)[:, 0] if x.ndim == 1 else A[:, :1] * 0 + x[:1] * 0
    for k in _index(A.shape[1], order):
        acc = acc + (A[:, k] * x[k] if x.ndim == 1 else A[:, k][:, None] * x[k][None, :])
    return acc


def _dot(a, b, order="numpy"):
    if order == "numpy":
        return a @ b
    s = a[0] * 0
    for k in _index(len(a), order):
        s = s + a[k] * b[k]
    return s


def _vectors(x, Z, W, lam, sf, noise, Binv, prec, order):
    k = kernel(Z, np.asarray(x).reshape(1, -1), lam, sf, prec)[:, 0]
    v = _mv(W, k, order)
    Lam = sf * sf + noise - _dot(v, v, order)
    return v, Lam, _mv(Binv, v, order)


def _cast(prec, *arrays):
    return (cast(a, prec) for a in arrays)


def append(x, y, Z, W, lam, sf, noise, G, r, Binv, Q, prec=None, order="numpy"):
    """``R.append`` with the summation order of its dot products chosen."""
    W, G, r, Binv, Q, y, sf, noise = _cast(prec, W, G, r, Binv, Q, np.asarray(y).reshape(-1), sf, noise)
    v, Lam, t = _vectors(x, Z, W, lam, sf, noise, Binv, prec, order)
    den = Lam + _dot(v, t, order)
    u = _mv(W.T, t, order)
    G, r = G + np.outer(v, v) / Lam, r + np.outer(v, y) / Lam
    Binv, Q = Binv - np.outer(t, t) / den, Q + np.outer(u, u) / den
    return {"G": G, "r": r, "Binv": Binv, "Q": Q, "alpha": _mv(W.T, _mv(Binv, r, order), order), "Lambda": Lam, "den": den}


def remove(x, y, Z, W, lam, sf, noise, G, r, Binv, Q, prec=None, order="numpy", mistake=None):
    """One held observation out, by the rank-one formulas; returns the updated G, r, Binv, Q, alpha, and Lambda, den.
    mistake "den_plus": den = Lambda + v . t (the append's); "r_kept": r not updated (for the discrimination tests)."""
    W, G, r, Binv, Q, y, sf, noise = _cast(prec, W, G, r, Binv, Q, np.asarray(y).reshape(-1), sf, noise)
    v, Lam, t = _vectors(x, Z, W, lam, sf, noise, Binv, prec, order)
    den = Lam + _dot(v, t, order) if mistake == "den_plus" else Lam - _dot(v, t, order)
    u = _mv(W.T, t, order)
    G = G - np.outer(v, v) / Lam
    if mistake != "r_kept":
        r = r - np.outer(v, y) / Lam
    Binv, Q = Binv + np.outer(t, t) / den, Q - np.outer(u, u) / den
    return {"G": G, "r": r, "Binv": Binv, "Q": Q, "alpha": _mv(W.T, _mv(Binv, r, order), order), "Lambda": Lam, "den": den}


def replace(x_old, y_old, x_new, y_new, Z, W, lam, sf, noise, G, r, Binv, Q, prec=None, order="numpy"):
    """remove(x_old, y_old) then append(x_new, y_new), the plain way; "Lambda" is the new row's."""
    s = remove(x_old, y_old, Z, W, lam, sf, noise, G, r, Binv, Q, prec, order)
    return append(x_new, y_new, Z, W, lam, sf, noise, s["G"], s["r"], s["Binv"], s["Q"], prec, order)


def replace_fused(x_old, y_old, x_new, y_new, Z, W, lam, sf, noise, G, r, Binv, Q, prec=None, order="numpy", mistake=None):
    """The route of gpmpc_sparse_replace: the removed state is not formed; t_n = s_n + c t_o with s_n = Binv v_n, c = (t_o . v_n) / den_o.
    mistake "tn_uncorrected": t_n = s_n."""
    W, G, r, Binv, Q, yo, yn, sf, noise = _cast(prec, W, G, r, Binv, Q, np.asarray(y_old).reshape(-1), np.asarray(y_new).reshape(-1), sf, noise)
    vo, Lo, to = _vectors(x_old, Z, W, lam, sf, noise, Binv, prec, order)
    vn, Ln, sn = _vectors(x_new, Z, W, lam, sf, noise, Binv, prec, order)
    den_o = Lo - _dot(vo, to, order)
    tn = sn if mistake == "tn_uncorrected" else sn + (_dot(to, vn, order) / den_o) * to
    den_n = Ln + _dot(vn, tn, order)
    uo, un = _mv(W.T, to, order), _mv(W.T, tn, order)
    G = (G - np.outer(vo, vo) / Lo) + np.outer(vn, vn) / Ln
    r = (r - np.outer(vo, yo) / Lo) + np.outer(vn, yn) / Ln
    Binv = (Binv + np.outer(to, to) / den_o) - np.outer(tn, tn) / den_n
    Q = (Q - np.outer(uo, uo) / den_o) + np.outer(un, un) / den_n
    return {"G": G, "r": r, "Binv": Binv, "Q": Q, "alpha": _mv(W.T, _mv(Binv, r, order), order), "Lambda": Ln, "den": den_n}


def _refresh(st, W, prec):
    st["Binv"] = R.inv_spd(R.eye_like(st["G"]) + st["G"])
    st.update(R.finish(W, st["Binv"], st["r"], prec))


def chain(X, Y, Z, W, lam, sf, noise, window, prec=None, order="numpy", refresh_every=64, rebase_every=0, trace=None):
    """Fit rows [0, window), then replace in ring order: row i takes the place of row i - window, i = window ... n - 1.  Counters as the
    state's: every ``refresh_every`` rank-one steps Binv is a fresh inverse of I + G (then alpha, Q); every ``rebase_every``
    replacements G and r are re-accumulated over the rows held, oldest first, and refreshed (which restarts the refresh count too).
    ``trace(i, state)`` is called after every replacement.  Returns G, r, Binv, Q, alpha."""
    X, Y = np.asarray(X), np.asarray(Y).reshape(len(X), -1)
    Wp = cast(W, prec)

    def batch(lo, hi):
        a = R.accumulate(X[lo:hi], Y[lo:hi], Z, W, lam, sf, noise, prec)
        st = {"G": a["G"], "r": a["r"]}
        _refresh(st, Wp, prec)
        return st
    st = batch(0, window)
    steps = since = 0
    for i in range(window, len(X)):
        o = i - window
        new = replace(X[o], Y[o], X[i], Y[i], Z, W, lam, sf, noise, st["G"], st["r"], st["Binv"], st["Q"], prec, order)
        st = {k: new[k] for k in ("G", "r", "Binv", "Q", "alpha")}
        steps, since = steps + 1, since + 1
        if refresh_every and steps >= refresh_every:
            _refresh(st, Wp, prec)
            steps = 0
        if rebase_every and since >= rebase_every:
            st = batch(o + 1, i + 1)
            steps = since = 0
        if trace is not None:
            trace(i, st)
    return st


def evaluations(fn, orders, *args, **kw):
    """[fn(*args, prec=float64, order=o) for o in orders]."""
    return [fn(*args, prec=np.float64, order=o, **kw) for o in orders]


def allowance4(ref_ld, f64_evaluations):
    """max(8 e64, 1e-13 max|ref|) with e64 the LARGEST max-abs error of the given float64 evaluations (the four ``ORDERS``) against the
    extended-precision one: one evaluation's error (``R.allowance``) is not a fair measure of a cancelling removal."""
    e64 = max(R.err(f, ref_ld) for f in f64_evaluations)
    return max(8.0 * e64, 1e-13 * R.max_abs(ref_ld))


OUTPUTS = ("G", "r", "Binv", "Q", "alpha")


def state64(pr):
    """The float64 state a kernel-level case starts from, as tests/test_gpu_sparse.py builds it for the append: G, r and Q rounded from the
    extended-precision evaluation on the case's W and Binv (symmetric)."""
    acc = R.accumulate(pr["X"], pr["Y"], pr["Z"], pr["W"], pr["lam"], pr["sf"], pr["noise"])
    G64, r64 = R.to_f64(acc["G"]), R.to_f64(acc["r"])
    G64 = (G64 + G64.T) / 2
    Q64 = R.to_f64(R.finish(pr["W"], pr["Binv"], r64)["Q"])
    Q64 = (Q64 + Q64.T) / 2
    return {"G": G64, "r": r64, "Binv": pr["Binv"], "Q": Q64, "min_lambda": float(acc["min_lambda"])}


def rows_of(n):
    """The rows a ladder case removes / replaces: the first, the middle and the last one."""
    return sorted({0, n // 2, n - 1})


@functools.lru_cache(maxsize=None)
def problem(M, n, D, nt):
    pr = R.problem(R.seed_of(M, n, D, nt), n, M, D, nt)
    return pr, state64(pr)


@functools.lru_cache(maxsize=None)
def case(M, n, D, nt, j):
    """Row j of the ladder case removed, and replaced by (xnew, ynew): the extended-precision evaluation ("ld") and the four float64
    evaluations ("f64", in ``ORDERS``) of ``remove`` and ``replace`` on the float64 state of the case.  Computed once."""
    pr, st = problem(M, n, D, nt)
    tail = (pr["Z"], pr["W"], pr["lam"], pr["sf"], pr["noise"], st["G"], st["r"], st["Binv"], st["Q"])
    rem = (pr["X"][j], pr["Y"][j]) + tail
    rep = (pr["X"][j], pr["Y"][j], pr["xnew"], pr["ynew"]) + tail
    return {"rem_args": rem, "rep_args": rep,
            "rem": {"ld": remove(*rem), "f64": evaluations(remove, ORDERS, *rem)},
            "rep": {"ld": replace(*rep), "f64": evaluations(replace, ORDERS, *rep)}}
