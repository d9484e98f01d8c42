"""Holds tests/sparse_window_reference.py itself and everything of the sparse-GP window that needs no device (CPU):

  * the C ABI of gpmpc_sparse_remove / gpmpc_sparse_replace: names, signatures, workspace sizes, the refusals before any launch;
  * the reference is right: a removal equals the extended-precision fit of the other rows, a replacement the fit of the swapped set,
    both also against the direct (unwhitened) FITC definition in mpmath; remove after append returns the state;
  * the allowance rule of the GPU tests (``allowance4``: 8 x the largest error of four float64 evaluations in different summation
    orders) holds for float64 evaluations it has not seen, the fused route of the device's replace among them, on the whole ladder;
  * three deliberate mistakes miss that allowance a hundred-fold;
  * argument errors of ``SparseDynamics(window=...)`` that come before the device is needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import sparse_reference as R
import sparse_window_reference as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gpmpc_sparse_remove_workspace_bytes", "gpmpc_sparse_remove", "gpmpc_sparse_replace_workspace_bytes", "gpmpc_sparse_replace"]
E_ARG, E_WORKSPACE = -1, -4


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_mpc_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_abi_names_and_signatures(L):
    from gaussian_process_mpc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    plain = (ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t, ctypes.POINTER(ctypes.c_double))
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        res, args = _lib.SIGNATURES[name]
        assert res in (ctypes.c_int, ctypes.c_size_t) and all(a in plain for a in args), name
        assert getattr(L, name) is not None
        n_decl = len(re.search(r"\b%s\s*\((.*?)\);" % name, hdr, flags=re.S).group(1).split(","))
        assert n_decl == len(args), (name, n_decl, len(args))


def test_workspace_sizes(L):
    for M, nt in ((1, 1), (33, 2), (130, 8), (1024, 4)):
        assert L.gpmpc_sparse_replace_workspace_bytes(M, nt) >= 8 * (7 * M + M * nt)
        assert L.gpmpc_sparse_remove_workspace_bytes(M, nt) >= L.gpmpc_sparse_append_workspace_bytes(M, nt) > 0
    for fn in (L.gpmpc_sparse_remove_workspace_bytes, L.gpmpc_sparse_replace_workspace_bytes):
        assert fn(0, 2) == 0 and fn(8193, 2) == 0 and fn(8, 0) == 0 and fn(8, 9) == 0


def test_refusals_before_any_launch(L):
    """Decided on the host, from sizes and pointers: GPMPC_E_ARG with the entry point's name leading the text (this runs without a device)."""
    from gaussian_process_mpc_amd._lib import host_doubles
    lam = host_doubles(np.ones(8))[1]
    p = ctypes.c_void_p(4096)                                               # never dereferenced: every call below is refused first

    def rem(D=3, M=8, nt=2, x=p, y=p, Z=p, W=p, ld_w=8, lam=lam, G=p, r=p, Binv=p, Q=p, alpha=p, st=p, ws=p, nb=1 << 30):
        return L.gpmpc_sparse_remove(D, M, nt, x, y, Z, W, ld_w, lam, 1.0, 1e-2, G, r, Binv, Q, alpha, st, ws, nb, None)

    def rep(D=3, M=8, nt=2, x=p, y=p, xn=p, yn=p, Z=p, W=p, ld_w=8, lam=lam, G=p, r=p, Binv=p, Q=p, alpha=p, st=p, ws=p, nb=1 << 30):
        return L.gpmpc_sparse_replace(D, M, nt, x, y, xn, yn, Z, W, ld_w, lam, 1.0, 1e-2, G, r, Binv, Q, alpha, st, ws, nb, None)

    sizes = [dict(M=0), dict(M=8193, ld_w=8193), dict(D=9), dict(nt=9), dict(ld_w=7)]
    pointers = ["x", "y", "Z", "W", "lam", "G", "r", "Binv", "Q", "alpha", "st", "ws"]
    for fn, name, extra in ((rem, "gpmpc_sparse_remove", []), (rep, "gpmpc_sparse_replace", ["xn", "yn"])):
        for kw in sizes + [{k: None} for k in pointers + extra]:
            assert fn(**kw) == E_ARG, (name, kw)
            assert L.gpmpc_last_error().decode().startswith(name), (name, kw, L.gpmpc_last_error())
        assert "NULL" in L.gpmpc_last_error().decode()
        assert fn(nb=getattr(L, name + "_workspace_bytes")(8, 2) - 1) == E_WORKSPACE


def test_window_argument_errors(L):
    """Argument errors come before the device is needed."""
    import gaussian_process_mpc_amd as g
    Z = np.zeros((4, 3))
    for bad in (0, -3, 2.5, "8", True):
        with pytest.raises(ValueError, match="window"):
            g.SparseDynamics(2, 1, Z, window=bad)
    with pytest.raises(ValueError, match="keep_data"):
        g.SparseDynamics(2, 1, Z, window=8, keep_data=False)


# ------------------------------------------------------------------------------------------------------------------ the reference is right
def _rel(a, b):
    return R.err(a, b) / max(R.max_abs(b), 1e-300)


def test_remove_and_replace_equal_the_batch_fit_extended_precision():
    """Row j out of a fit of n rows against the fit of the other n - 1; row j replaced against the fit of the swapped set; remove after
    append against the state it started from.  Extended precision, to 1e-13 of the largest entry (64-bit mantissa: 5e-20, times the
    cancellation Lambda / den <= 1e3 of a removal and the condition of B, 1e3 here: far below)."""
    pr = R.problem(11, 120, 24, 3, 2)
    hyp = (pr["lam"], pr["sf"], pr["noise"])
    full = R.fit(pr["X"], pr["Y"], pr["Z"], *hyp, pr["jitter"], W=pr["W"])
    state = tuple(full[k] for k in ("G", "r", "Binv", "Q"))
    for j in (0, 60, 119):
        keep = [i for i in range(pr["n"]) if i != j]
        less = R.fit(pr["X"][keep], pr["Y"][keep], pr["Z"], *hyp, pr["jitter"], W=pr["W"])
        got = WR.remove(pr["X"][j], pr["Y"][j], pr["Z"], pr["W"], *hyp, *state)
        Xs, Ys = np.array(pr["X"]), np.array(pr["Y"])
        Xs[j], Ys[j] = pr["xnew"], pr["ynew"]
        swapped = R.fit(Xs, Ys, pr["Z"], *hyp, pr["jitter"], W=pr["W"])
        plain = WR.replace(pr["X"][j], pr["Y"][j], pr["xnew"], pr["ynew"], pr["Z"], pr["W"], *hyp, *state)
        fused = WR.replace_fused(pr["X"][j], pr["Y"][j], pr["xnew"], pr["ynew"], pr["Z"], pr["W"], *hyp, *state)
        for k in WR.OUTPUTS:
            e = (_rel(got[k], less[k]), _rel(plain[k], swapped[k]), _rel(fused[k], swapped[k]))
            print("  row %3d %-5s remove %.2e replace %.2e fused replace %.2e (relative)" % ((j, k) + e))
            assert max(e) <= 1e-13, (j, k, e)
    app = R.append(pr["xnew"], pr["ynew"], pr["Z"], pr["W"], *hyp, *state)
    back = WR.remove(pr["xnew"], pr["ynew"], pr["Z"], pr["W"], *hyp, *(app[k] for k in ("G", "r", "Binv", "Q")))
    for k in WR.OUTPUTS:
        assert _rel(back[k], full[k]) <= 1e-13, k


@pytest.mark.parametrize("seed,n,M,D,nt,j", [(3, 20, 8, 3, 2, 7), (4, 12, 5, 2, 1, 0)])
def test_remove_and_replace_equal_direct_fitc_mpmath(seed, n, M, D, nt, j):
    import mpmath as mp
    with mp.workprec(100):
        pr = R.problem(seed, n, M, D, nt)
        hyp = (pr["lam"], pr["sf"], pr["noise"])
        w = R.fit(pr["X"], pr["Y"], pr["Z"], *hyp, pr["jitter"], prec=R.MP)
        state = tuple(w[k] for k in ("G", "r", "Binv", "Q"))
        keep = [i for i in range(n) if i != j]
        Xs, Ys = np.array(pr["X"]), np.array(pr["Y"])
        Xs[j], Ys[j] = pr["xnew"], pr["ynew"]
        rem = WR.remove(pr["X"][j], pr["Y"][j], pr["Z"], w["W"], *hyp, *state, prec=R.MP)
        rep = WR.replace(pr["X"][j], pr["Y"][j], pr["xnew"], pr["ynew"], pr["Z"], w["W"], *hyp, *state, prec=R.MP)
        d_rem = R.direct_fitc(pr["X"][keep], pr["Y"][keep], pr["Z"], *hyp, pr["jitter"], prec=R.MP)
        d_rep = R.direct_fitc(Xs, Ys, pr["Z"], *hyp, pr["jitter"], prec=R.MP)
        for k in ("alpha", "Q"):
            e = (_rel(rem[k], d_rem[k]), _rel(rep[k], d_rep[k]))
            print("  against direct FITC, %s: remove %.2e replace %.2e relative" % ((k,) + e))
            assert max(e) <= 1e-15, (k, e)


# ------------------------------------------------------------------------------------------------------------------ the allowance rule
def _ratios(ld, f64s, other):
    return {k: R.err(other[k], ld[k]) / WR.allowance4(ld[k], [f[k] for f in f64s]) for k in WR.OUTPUTS}


@pytest.mark.parametrize("M,n,D,nt", R.ladder())
def test_allowance_rule_holds_for_unseen_float64_evaluations(M, n, D, nt):
    """Float64 evaluations the allowance has not seen -- three more permutations, and for the replace the device's fused route in the
    four orders and one more -- stay within it on every output of every ladder case and row."""
    worst = {}
    for j in WR.rows_of(n):
        c = WR.case(M, n, D, nt, j)
        held = [("remove %r" % (o,), "rem", WR.remove(*c["rem_args"], prec=np.float64, order=o)) for o in WR.HELD_OUT]
        held += [("replace %r" % (o,), "rep", WR.replace(*c["rep_args"], prec=np.float64, order=o)) for o in WR.HELD_OUT]
        held += [("fused %r" % (o,), "rep", WR.replace_fused(*c["rep_args"], prec=np.float64, order=o)) for o in WR.ORDERS + WR.HELD_OUT[:1]]
        for label, what, ev in held:
            for k, q in _ratios(c[what]["ld"], c[what]["f64"], ev).items():
                key = (label.split()[0], k)
                worst[key] = max(worst.get(key, 0.0), q)
                assert q <= 1.0, (label, j, k, q)
    print("  M %3d n %3d D %d nt %d: worst held-out error / allowance4 " % (M, n, D, nt)
          + ", ".join("%s %s %.2f" % (a, k, q) for (a, k), q in sorted(worst.items()) if q >= 0.2))


@pytest.mark.parametrize("mistake", ["den_plus", "r_kept", "tn_uncorrected"])
def test_mistakes_miss_the_allowance_hundredfold(mistake):
    """den = Lambda + v . t in the removal, r not updated, t_n = s_n without the correction: some output misses allowance4 by >= 100 x."""
    M, n, D, nt = 33, 200, 5, 4
    c = WR.case(M, n, D, nt, n // 2)
    if mistake == "tn_uncorrected":
        bad, what = WR.replace_fused(*c["rep_args"], prec=np.float64, mistake=mistake), "rep"
    else:
        bad, what = WR.remove(*c["rem_args"], prec=np.float64, mistake=mistake), "rem"
    q = _ratios(c[what]["ld"], c[what]["f64"], bad)
    print("  %s: error / allowance4 " % mistake + ", ".join("%s %.3g" % kv for kv in q.items()))
    assert max(q.values()) >= 100.0


def test_allowance4_rule():
    a = np.array([1.0, -3.0], dtype=R.LD)
    same = np.array([1.0, -3.0])
    assert WR.allowance4(a, [same, same]) == 1e-13 * 3.0
    assert WR.allowance4(a, [same, np.array([1.0 + 1e-10, -3.0]), np.array([1.0, -3.0 - 3e-10])]) == pytest.approx(24e-10, rel=1e-3)
