"""Host side of the rounding-error budget of single-step moment matching (tests/moment_reference.py, tests/test_gpu_moment.py): no GPU.

1. The yardstick is pinned: the long double step and its complex-step Jacobians (oracle/cport/gpmpc_cpu_given.c) against the mpmath
   restatement at 50 digits (N <= 6, D <= 3, ds <= 2, both covariance forms) -- within 0.75 unit: the entries are returned rounded to
   double, half an ulp of the value, at most half a unit, and the long double evaluation itself (expl of a rounded quadratic form) is
   allowed a quarter; measured: 0.53 for l, below 0.5 elsewhere -- and against CPU torch autograd of oracle/gpmpc_oracle.py on
   the instances, at the fp64 floor of that evaluation (recorded below).
2. The input conditions of every table the GPU tests run are asserted from the long double values.
3. K_ref, the K of the float64 emulation of the kernels' formulas, is recorded per output and case (printed).
4. The table of defects: each defect is emulated in float64 and judged twice -- by the bands and inputs of the tests that existed before
   (the g2 entries of GP 0 at D = 2 with sigma_f = 1 and shared targets at 1e-7 / 1e-5, dcov at 1e-6; ONE random direction at D = 6, 7 at
   rtol 2e-4; l at N < 256 at 1e-4), and by the budget K <= 10 max(K_ref, 0.5).

Measured here (x86-64, float64 emulation, K_ref per output over the tables; see `python -m pytest -s tests/test_host_moment.py`):
    families at (3, 2), N = 90       generic / correlated / zero / zero_row / skew 0.01 ... 3.7;  far 0.2 ... 4.0;
                                     stiff: l 12, every sum 5e-4 ... 5e-3 (the unit is a bound there: moment_reference.py)
    instances, N = 90                0.04 ... 3.7 (l 2 ... 3.7; Jacobians 0.05 ... 1.4)
    edges N = 1 ... 257 at (3, 2)    0.02 ... 3.4;  N = 2100, 1100: sums 0.002 ... 0.15, l 2.6
Defects: see test_what_the_budget_buys; three of the seven are gaps (the older judgement passes them, the budget fails them).
"""
import numpy as np
import pytest
import torch

import moment_reference as R
from oracle import cport
from oracle import gpmpc_oracle as O

_CONST = {}


def _consts(D, ds, N, **kw):
    key = (D, ds, N, tuple(sorted(kw.items())))
    if key not in _CONST:
        pb = R.problem(D, ds, N)
        if kw.get("g2"):                         # the setting of the g2 fixture: sigma_f = 1 and one target vector for every GP
            pb["sigma_f"] = np.ones(ds)
            pb["Y"] = np.repeat(pb["Y"][:, :1], ds, axis=1)
            pb = dict(pb, Ky_inv=np.stack([O.kernel_matrices(O._t(pb["X"]), O._t(pb["lambdas"][a]), 1.0, 0.1)[2].numpy() for a in range(ds)]))
        beta, W = cport.constants(pb, pb["Ky_inv"])
        _CONST[key] = (pb, beta, W)
    return _CONST[key]


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the yardstick
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bug", [False, True])
@pytest.mark.parametrize("D,ds,N,family", [(1, 1, 4, "generic"), (2, 2, 5, "generic"), (3, 2, 6, "generic"), (3, 2, 6, "correlated"),
                                           (2, 2, 5, "zero_row"), (3, 2, 4, "skew")])
def test_complex_step_against_mpmath(D, ds, N, family, bug):
    pb, beta, W = _consts(D, ds, N)
    u, S = R.queries(pb, family, 1)
    ref, A = R.reference(pb, beta, W, u, S, bug=bug)
    m = R.mp_step(pb, beta, W, u[0], S[0], bug=bug)
    m["var"] = np.array([m["cov"][a, a] for a in range(ds)], dtype=object)
    m["dvar_du"] = np.array([m["dcov_du"][a, a] for a in range(ds)], dtype=object)
    m["dvar_dS"] = np.array([m["dcov_dS"][a, a] for a in range(ds)], dtype=object)
    worst = {}
    for k in R.OUTPUTS:
        r, a, t = ref[k][0].reshape(-1), A[k][0].reshape(-1), m[k].reshape(-1)
        worst[k] = max(float(abs(t[i] - float(r[i])) / (2.0 ** -53 * max(a[i], R.TINY))) for i in range(r.size))
    print("PIN mpmath D=%d ds=%d N=%d %s %s: %s" % (D, ds, N, family, "bug" if bug else "consistent", "  ".join("%s %.3g" % kv for kv in worst.items())))
    for k, v in worst.items():
        assert v <= 0.75, (k, v)


def _autograd(pb, beta, u, S, bug):
    """mean, var, cov and their Jacobians (d/dS symmetrised) of oracle/gpmpc_oracle.py by CPU torch autograd, on the given beta."""
    X, lam, sf, Kinv = O._t(pb["X"]), O._t(pb["lambdas"]), pb["sigma_f"], O._t(pb["Ky_inv"])
    ds, D = pb["ds"], X.shape[1]
    b = O._t(beta[:, :X.shape[0]])

    def f(ut, St):
        Ss = 0.5 * (St + St.mT)
        mu, var = [], []
        for a in range(ds):
            _, _, l = O.mean_prop(Kinv[a], lam[a], ut, Ss, X, O._t(pb["Y"][:, a]), float(sf[a]))
            mu.append(torch.dot(b[a], l))
            L = O._pair_matrix_L(lam[a], ut, Ss, X, float(sf[a]))
            var.append(float(sf[a]) ** 2 - torch.sum((0.5 * (Kinv[a] + Kinv[a].mT) - torch.outer(b[a], b[a])) * L.mT) - mu[a] ** 2)
        out = list(mu)
        for a in range(ds):
            for c in range(ds):
                out.append(var[a] if a == c else O.covariance_prop(lam[a], lam[c], ut, Ss, X, mu[a], mu[c], b[a], b[c], float(sf[a]),
                                                                   float(sf[c]), bug_compatible=bug))
        return torch.stack(out)
    ut, St = O._t(u).clone().requires_grad_(True), O._t(S).clone().requires_grad_(True)
    Ju, JS = torch.autograd.functional.jacobian(f, (ut, St))
    JS = 0.5 * (JS + JS.mT)
    Ju, JS = Ju.numpy(), JS.numpy()
    return {"dmean_du": Ju[:ds], "dmean_dS": JS[:ds], "dcov_du": Ju[ds:].reshape(ds, ds, D), "dcov_dS": JS[ds:].reshape(ds, ds, D, D)}


@pytest.mark.parametrize("D,ds", R.INSTANCES)
def test_complex_step_against_autograd_of_the_oracle(D, ds):
    """Another derivation of the same Jacobians (reverse mode through torch.linalg.inv / det), in plain float64: held like any float64
    evaluation, K <= 10 max(K_ref, 0.5) with K_ref of the emulation on the same query.  Measured: K up to 0.9 (K_ref up to 1.4)."""
    N = 30
    pb, beta, W = _consts(D, ds, N)
    u, S = R.queries(pb, "generic", 1)
    for bug in (False, True) if ds > 1 else (False,):
        ref, A = R.reference(pb, beta, W, u, S, bug=bug)
        got = _autograd(pb, beta, u[0], S[0], bug)
        ks = {k: R.k_of(got[k], ref[k][0], A[k][0]) for k in got}
        kref = R.k_all(R.emulate(pb, beta, W, u[0], S[0], bug=bug, cross="direct"), ref, A, 0)
        print("PIN autograd D=%d ds=%d N=%d %s: %s" % (D, ds, N, "bug" if bug else "consistent",
                                                       "  ".join("%s %.3g (%.3g)" % (k, v, kref[k]) for k, v in ks.items())))
        for k, v in ks.items():
            assert v <= 10.0 * max(kref[k], 0.5), (k, v, kref[k])


# ------------------------------------------------------------------------------------------------------------------------------
# 2. input conditions, 3. K_ref
# ------------------------------------------------------------------------------------------------------------------------------
def _tables():
    """(D, ds, N, family, nq) of every call shape of tests/test_gpu_moment.py (the large-N cases apart: test_large_cases)."""
    t = [(D, ds, R.N_DEFAULT, "generic", 3) for D, ds in R.INSTANCES]
    t += [(3, 2, N, "generic", 2) for N in R.EDGE_N]
    t += [(3, 2, R.N_DEFAULT, f, 2) for f in R.FAMILIES]
    return t


def test_input_conditions_and_K_ref():
    kappa, rows = [], []
    for D, ds, N, family, nq in _tables():
        pb, beta, W = _consts(D, ds, N)
        u, S = R.queries(pb, family, nq)
        Ss = R.sym(S)
        ref, A = R.reference(pb, beta, W, u, S)
        assert np.all(ref["var"] > 0), (D, ds, N, family)
        for q in range(nq):
            assert np.all(np.linalg.eigvalsh(ref["cov"][q]) > 0), (D, ds, N, family, q)
            assert np.all(np.linalg.eigvalsh(Ss[q]) >= -1e-18)
            for a in range(ds):
                kappa.append(np.linalg.cond(Ss[q] + np.diag(pb["lambdas"][a])))
        if family == "correlated" and D > 1:
            d = np.sqrt(np.diagonal(Ss, axis1=1, axis2=2))
            rho = Ss / d[:, :, None] / d[:, None, :]
            assert np.all(np.abs(rho) >= 0.9)
        if family == "skew":
            assert np.abs(S - Ss).max() > 1e-4
        if family == "far":
            for q in range(nq):
                for a in range(ds):
                    v = u[q] - pb["X"]
                    ex = -0.5 * ((v @ np.linalg.inv(Ss[q] + np.diag(pb["lambdas"][a]))) * v).sum(1)
                    assert ex.max() < -10.0 and ex.min() > -700.0, (ex.max(), ex.min())
            assert np.all(ref["mean"] != 0.0) and np.all(ref["l"] > 0.0)                   # nothing underflows in the mean sum
        if family == "zero":
            assert not S.any()
            for a in range(ds):
                B, det = R.gj_nopivot(Ss[0] + np.diag(pb["lambdas"][a]))
                assert np.array_equal(B, np.diag(1.0 / pb["lambdas"][a]))                   # S = 0: B is Lambda^-1 exactly
        if family == "zero_row":
            assert not S[:, 0, :].any() and not S[:, :, 0].any() and (D == 1 or S[:, 1:, 1:].any())
        if ds > 1 and R.bug_held(family, N):
            # the bug-compatible covariance is another number wherever a test means to hold it (moment_reference.bug_held)
            refb, _ = R.reference(pb, beta, W, u, S, bug=True)
            off = ~np.eye(ds, dtype=bool)
            for q in range(nq):
                gap = np.abs(refb["cov"][q] - ref["cov"][q])[off] / (2.0 ** -53 * A["cov"][q][off])
                assert gap.min() > 1e6, (D, ds, N, family, q, gap.min())
        for cross in ("direct", "pair") if ds > 1 else ("direct",):
            ks = [R.k_all(R.emulate(pb, beta, W, u[q], S[q], cross=cross), ref, A, q) for q in range(nq)]
            k = {n: max(x[n] for x in ks) for n in ks[0]}
            rows.append("K_ref D=%d ds=%d N=%-3d %-10s %-6s %s" % (D, ds, N, family, cross, "  ".join("%s %.2g" % kv for kv in k.items())))
            for n, v in k.items():      # the emulation IS the kernels' formulas in float64: it stays inside the budget's scale on every case
                assert v <= 20.0, (D, ds, N, family, cross, n, v)
    print("\n" + "\n".join(rows))
    assert min(kappa) < 1.0 + 1e-12 and max(kappa) > 1e3, (min(kappa), max(kappa))


@pytest.mark.parametrize("D,ds,N", R.LARGE)
def test_large_cases(D, ds, N):
    """The rows past one trip of the mean loop carry weight: the mean changes by more than 1e6 units without them."""
    pb, beta, W = _consts(D, ds, N)
    u, S = R.queries(pb, "generic", 1)
    ref, A = R.reference(pb, beta, W, u, S)
    trip = 2 * (4 if D <= 5 else 2) * 256
    assert N > trip
    em = R.emulate(pb, beta, W, u[0], S[0])
    print("K_ref D=%d ds=%d N=%d generic: %s" % (D, ds, N, "  ".join("%s %.2g" % kv for kv in R.k_all(em, ref, A, 0).items())))
    b2 = beta.copy()
    b2[:, trip:] = 0.0
    cut = R.emulate(pb, b2, W, u[0], S[0], want_var=False)
    assert R.k_of(cut["mean"], ref["mean"][0], A["mean"][0]) > 1e6


# ------------------------------------------------------------------------------------------------------------------------------
# 4. what the budget buys
# ------------------------------------------------------------------------------------------------------------------------------
def _close(a, b, rtol, atol):
    return bool(np.all(np.abs(a - b) <= atol + rtol * np.abs(b)))


def _old_judgement(defect):
    """True when the tests that existed before would have PASSED this defect: their inputs and bands, the defective emulation against the
    sound one (at those bands the sound emulation is the truth)."""
    cross = "pair"
    ok = True
    # g2: D = 2, ds = 2, sigma_f = 1, shared targets; mean / var / cov, the Jacobians of GP 0 only, dcov of the one pair
    pb, beta, W = _consts(2, 2, 8, g2=True)
    u, S = R.queries(pb, "generic", 2)
    for q in range(2):
        bad, good = (R.emulate(pb, beta, W, u[q], S[q], cross=cross, defect=d) for d in (defect, None))
        ok &= _close(bad["mean"], good["mean"], 1e-9, 1e-12) and _close(bad["cov"], good["cov"], 1e-6, 1e-12)
        for k in ("dmean_du", "dmean_dS", "dvar_du", "dvar_dS"):
            ok &= _close(bad[k][0], good[k][0], 1e-5, 1e-7)
        if cross == "pair":
            ok &= _close(bad["dcov_du"][0, 1], good["dcov_du"][0, 1], 1e-6, 1e-9) and _close(bad["dcov_dS"][0, 1], good["dcov_dS"][0, 1], 1e-6, 1e-9)
        ok &= _close(bad["l"], good["l"], 1e-4, 1e-12)
    # the direct kernel's dcov in the reference's (bug-compatible) form against stored autograd values at D = 2, sigma_f != 1, rtol 1e-6
    # (tests/test_gpu_autograd.py::test_covariance_prop_torch_carries_the_graph); the cov values of g1 / g2 at 1e-6
    pb, beta, W = _consts(2, 2, 8)
    u, S = R.queries(pb, "generic", 2)
    for q in range(2):
        bad, good = (R.emulate(pb, beta, W, u[q], S[q], bug=True, cross="direct", defect=d) for d in (defect, None))
        ok &= _close(bad["cov"], good["cov"], 1e-6, 1e-12)
        ok &= _close(bad["dcov_du"][0, 1], good["dcov_du"][0, 1], 1e-6, 1e-9) and _close(bad["dcov_dS"][0, 1], good["dcov_dS"][0, 1], 1e-6, 1e-9)
    # one random direction at D = 6, 7: dmean and dvar of every GP along it, rtol 2e-4
    for D, ds in ((6, 3), (7, 2)):
        pb, beta, W = _consts(D, ds, R.N_DEFAULT)
        u, S = R.queries(pb, "generic", 1)
        rng = np.random.default_rng(D)
        du, dS = rng.normal(size=D), rng.normal(size=(D, D))
        dS = 0.5 * (dS + dS.T)
        bad, good = (R.emulate(pb, beta, W, u[0], S[0], cross="direct", defect=d) for d in (defect, None))
        for m in ("mean", "var"):
            g = [x["d%s_du" % m] @ du + np.einsum("akl,kl->a", x["d%s_dS" % m], dS) for x in (bad, good)]
            ok &= _close(g[0], g[1], 2e-4, 1e-10)
    return ok


def _budget_judgement(defect):
    """True when the budget of tests/test_gpu_moment.py would have PASSED it on one of its own cases."""
    D, ds, N = (3, 2, 257) if defect == "l_row_256" else (3, 2, R.N_DEFAULT)
    pb, beta, W = _consts(D, ds, N)
    u, S = R.queries(pb, "generic", 2)
    ref, A = R.reference(pb, beta, W, u, S)
    ok = True
    for cross in ("pair", "direct"):
        for q in range(2):
            kref = R.k_all(R.emulate(pb, beta, W, u[q], S[q], cross=cross), ref, A, q)
            k = R.k_all(R.emulate(pb, beta, W, u[q], S[q], cross=cross, defect=defect), ref, A, q)
            ok &= all(k[n] <= 10.0 * max(kref[n], 0.5) for n in k)
    return ok


# True: a gap -- the older tests pass the defect.  Three of the seven: the older suite holds more than its g2 / one-direction bands suggest
# (the direct kernel's Jacobians against stored autograd values at D = 2 with sigma_f != 1, tests/test_gpu_autograd.py), so the amplitudes,
# R^-T for R^-1 and the dropped mean terms do not get past it; the run of the corresponding kernel mutations says the same.
EXPECTED_GAP = {"dvar_dS_gp1": True, "no_amplitudes": False, "no_mean_terms_dS": False, "z_for_zt": False, "factor_4_for_2": False,
                "rel_1e-5": True, "l_row_256": True}


def test_what_the_budget_buys():
    rows, gaps = [], {}
    for defect in R.DEFECTS:
        old, new = _old_judgement(defect), _budget_judgement(defect)
        assert not new, defect                                  # the budget fails every defect of the table
        gaps[defect] = bool(old)
        rows.append("DEFECT %-18s older tests: %-6s budget: %-6s %s" % (defect, "pass" if old else "FAIL", "pass" if new else "FAIL",
                                                                        "GAP" if old else "no gap"))
    print("\n" + "\n".join(rows))
    assert gaps == EXPECTED_GAP, rows
