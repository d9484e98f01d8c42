"""Holds tests/linprop_fc_reference.py itself and everything of the full-covariance linearised propagation that needs no device (CPU):

  * the reference's packed Jacobian equals torch.autograd.functional.jacobian of a float64 restatement of the value, taken with respect to
    the p packed variables with Sigma rebuilt symmetric from them, within the budget the GPU tests use (1e-12 sum |terms| carried through
    the composite outputs, plus 4 ulp of the sizes the last float64 additions round at), with and without a gain;
  * with K = None and a diagonal Sigma, the diagonal of Sigma' and the matching Jacobian entries are those of linprop_reference.step;
  * closed forms on a model without GP mean (beta = 0) and a linear nominal model;
  * each deliberate mistake of the reference misses that budget by at least 100: the budget discriminates;
  * the C ABI: names, signatures, exports, and every refusal of the header, which comes back as GPMPC_E_ARG without a device -- before any
    launch (check_refusals is also called by tests/test_gpu_linprop_fc.py);
  * the Riccati recursion behind lqr_gain."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import linprop_fc_reference as F
import linprop_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gpmpc_linearised_fc_step_workspace_bytes", "gpmpc_linearised_fc_step", "gpmpc_linearised_fc_rollout_workspace_bytes",
         "gpmpc_linearised_fc_rollout", "gpmpc_linearised_fc_vjp", "gpmpc_linearised_fc_constraints"]
E_ARG, E_WORKSPACE = -1, -4
TOL = 1e-12
ULP = 2.0 ** -52
f64 = R.G.to_f64


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_mpc_amd import _lib
    return _lib.lib()


def bound(ref, key):
    """tol * budget + 4 ulp of the magnitudes, float64."""
    return TOL * f64(ref[key + "_abs"]) + 4.0 * ULP * f64(ref[key + "_mag"])


# ------------------------------------------------------------------------------------------------------------------ the reference itself
def value_f64(model, x, K):
    """The packed (mu', Sigma'_ab for a <= b) of ONE column from the packed x = (mu, Sigma_kl for k <= l, v) in float64 torch.  g is written
    out; its derivative (the Hessian terms) is autograd's.  Sigma is rebuilt symmetric from the packed variables."""
    ds, da, D = R.dims(model)
    _, av, pv = R.noise_model(model)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    pairs = F.tri_pairs(ds)
    p = F.packed_dim(ds)
    mu, v = x[:ds], x[p:]
    S = torch.zeros((ds, ds), dtype=torch.float64)
    rows = [[None] * ds for _ in range(ds)]
    for c, (k, l) in enumerate(pairs):
        rows[k][l] = rows[l][k] = x[ds + c]
    S = torch.stack([torch.stack(r) for r in rows])
    z = torch.cat([mu, v])
    X, beta = t(model["X"]), t(model["beta"])
    ms, gs, s2 = [], [], []
    for a in range(ds):
        lam, sf = t(model["lam"][a]), float(model["sf"][a])
        diff = X - z[None, :]
        k = sf * sf * torch.exp(-0.5 * (diff * diff / lam[None, :]).sum(1))
        bk = beta[:, a] * k
        m = bk.sum()
        g = (bk[:, None] * diff / lam[None, :]).sum(0)
        if model.get("nominal") is not None:
            W, b = t(model["nominal"][0])[a], float(np.broadcast_to(model["nominal"][1], (ds,))[a])
            m = m + W @ z + b
            g = g + W
        Ki = t(R.P._kinv(model, a))
        ms.append(m)
        gs.append(g)
        s2.append(sf * sf - k @ (Ki @ k) + float(pv[a]))
    Gm = torch.stack(gs)                                                     # (ds, D)
    T = torch.cat([torch.eye(ds, dtype=torch.float64), t(K).reshape(da, ds) if K is not None else torch.zeros((da, ds), dtype=torch.float64)])
    Sz = T @ S @ T.T + torch.diag(torch.cat([torch.zeros(ds, dtype=torch.float64), t(av).reshape(-1)]))
    Sn = torch.diag(torch.stack(s2)) + Gm @ Sz @ Gm.T
    return torch.stack(ms + [Sn[a, b] for a, b in pairs])


CASES = {"pergp": lambda: R.make_model(40, 2, 1),
         "nonsym_nominal_noise": lambda: R.make_model(33, 3, 2, "nonsym", noise=True, nominal=True)}


@pytest.mark.parametrize("gain", [False, True], ids=["open_loop", "feedback"])
@pytest.mark.parametrize("case", list(CASES))
def test_reference_jacobian_is_autograd_of_its_value(case, gain):
    m = CASES[case]()
    ds, da, _ = R.dims(m)
    mu, cov, U, K = F.make_inputs(m, 2, gain=gain)
    ref = F.step(m, mu, cov, U, K)
    p = F.packed_dim(ds)
    worst = 0.0
    for c in range(2):
        x = torch.as_tensor(np.concatenate([F.pack_state(mu[c], cov[c]), U[c]]))
        val = value_f64(m, x, K).numpy()
        J = torch.autograd.functional.jacobian(lambda y: value_f64(m, y, K), x).numpy()
        assert J.shape == (p, p + da)
        want = f64(F.pack_state(ref["mu"][c], ref["cov"][c]))
        bv = np.concatenate([TOL * f64(ref["m_abs"][c]), f64(F.pack_state(np.zeros(ds), bound(ref, "cov")[c]))[ds:]])
        assert np.all(np.abs(val - want) <= bv)
        bj = bound(ref, "jac")[c]
        assert np.all((bj > 0) | ((J == 0) & (f64(ref["jac"][c]) == 0)))     # the structural zeros (d mu' / d Sigma) are zeros of both
        worst = max(worst, float((np.abs(J - f64(ref["jac"][c])) / np.where(bj > 0, bj, 1.0)).max()))
    print("  %s, %s: analytic packed Jacobian vs autograd, worst %.3g of the budget" % (case, "gain" if gain else "K = None", worst))
    assert worst <= 1.0


def test_diagonal_open_loop_is_the_diagonal_rule():
    m = R.make_model(50, 3, 2, noise=True, nominal=True)
    ds, da, D = R.dims(m)
    mu, var, U = R.make_inputs(m, 3)
    d = R.step(m, mu, var, U)
    cov = np.zeros((3, ds, ds))
    for k in range(ds):
        cov[:, k, k] = var[:, k]
    ref = F.step(m, mu, cov, U, None)
    bd = TOL * f64(d["var_abs"]) + 4 * ULP * f64(d["var_mag"])
    diag = lambda a: np.stack([a[:, k, k] for k in range(ds)], axis=1)  # noqa: E731
    ev = np.abs(f64(diag(ref["cov"]) - d["var"])) / (bd + diag(bound(ref, "cov")))
    pairs = F.tri_pairs(ds)
    p = F.packed_dim(ds)
    bj_d = TOL * f64(d["jac_abs"]) + 4 * ULP * f64(d["jac_mag"])
    bj_f = bound(ref, "jac")
    worst = 0.0
    for a in range(ds):
        row = ds + pairs.index((a, a))
        for dd in range(D):
            cf, cd = (dd if dd < ds else p + dd - ds), (dd if dd < ds else ds + dd)
            for rf, rd in ((a, a), (row, ds + a)):                           # the mu' row and the variance row, the zbar columns
                e = np.abs(f64(ref["jac"][:, rf, cf] - d["jac"][:, rd, cd])) / (bj_f[:, rf, cf] + bj_d[:, rd, cd])
                worst = max(worst, float(e.max()))
        for k in range(ds):                                                  # the Sigma_kk columns: g_ak^2
            cf = ds + pairs.index((k, k))
            e = np.abs(f64(ref["jac"][:, row, cf] - d["jac"][:, ds + a, ds + k])) / (bj_f[:, row, cf] + bj_d[:, ds + a, ds + k])
            worst = max(worst, float(e.max()))
    print("  K = None, diagonal Sigma: variance %.3g, Jacobian %.3g of the two budgets" % (ev.max(), worst))
    assert ev.max() <= 1.0 and worst <= 1.0


def _nominal_only(ds, da, seed=0):
    m = R.make_model(30, ds, da, noise=True, nominal=True, seed=seed)
    m["beta"] = np.zeros_like(m["beta"])
    return m


def test_closed_form_linear_model():
    """beta = 0 with a nominal (W, b): Sigma' = (A + B K) Sigma (A + B K)^T + B diag(action_var) B^T + diag(sf^2 - q + process_var); a gain
    with A + B K = 0 removes the Sigma term entirely."""
    m = _nominal_only(2, 2)
    ds, da, _ = R.dims(m)
    W = np.asarray(m["nominal"][0], dtype=np.float64)
    A, Bm = W[:, :ds], W[:, ds:]
    _, av, pv = R.noise_model(m)
    mu, cov, U, K = F.make_inputs(m, 3)
    ref = F.step(m, mu, cov, U, K)
    s2 = f64(np.asarray(m["sf"])[None, :] ** 2 - ref["base"]["q"] + np.asarray(pv)[None, :])
    Acl = A + Bm @ K
    want = np.einsum("ik,bkl,jl->bij", Acl, cov, Acl) + (Bm * np.asarray(av)[None, :]) @ Bm.T
    for a in range(ds):
        want[:, a, a] += s2[:, a]
    e = np.abs(f64(ref["cov"]) - want) / bound(ref, "cov")
    print("  closed form: %.3g of the budget" % e.max())
    assert e.max() <= 1.0
    K0 = -np.linalg.solve(Bm, A)
    r0 = F.step(m, mu, cov, U, K0)
    r1 = F.step(m, mu, 3.0 * cov, U, K0)
    want0 = np.broadcast_to((Bm * np.asarray(av)[None, :]) @ Bm.T, (3, ds, ds)).copy()
    for a in range(ds):
        want0[:, a, a] += s2[:, a]
    assert np.abs(f64(r0["P"])).max() <= 1e-15                               # the closed-loop gradient vanishes to the rounding of K0
    assert np.all(np.abs(f64(r0["cov"]) - want0) <= bound(r0, "cov") + 1e-15 * np.abs(cov).max())
    assert np.all(np.abs(f64(r0["cov"] - r1["cov"])) <= 1e-15 * np.abs(cov).max())
    pairs = F.tri_pairs(ds)
    assert np.abs(f64(r0["jac"][:, ds:, ds:ds + len(pairs)])).max() <= 1e-28  # products of two vanishing gradients


CONTROLS = ["drop_cross_hess", "feedback_cross_dropped", "offdiag_once"]


def control_factor(m, mu, cov, U, K, name):
    """By how many budgets the reference with mistake `name` misses the reference: the worst entry of Sigma' and the Jacobian."""
    ref, bad = F.step(m, mu, cov, U, K), F.step(m, mu, cov, U, K, **{name: True})
    bj = bound(ref, "jac")
    fj = np.abs(f64(bad["jac"] - ref["jac"])) / np.where(bj > 0, bj, np.inf)
    fv = np.abs(f64(bad["cov"] - ref["cov"])) / bound(ref, "cov")
    return max(float(fj.max()), float(fv.max()))


@pytest.mark.parametrize("name", CONTROLS)
def test_each_control_misses_the_budget(name):
    m = R.make_model(70, 2, 1)
    mu, cov, U, K = F.make_inputs(m, 3)
    assert np.abs(K).min() > 0 and np.abs(cov[:, 0, 1]).min() > 0            # a non-zero gain, a non-diagonal Sigma
    factor = control_factor(m, mu, cov, U, K, name)
    print("  control %s: misses by %.3g budgets" % (name, factor))
    assert factor >= 100.0


def test_feedback_shrinks_the_prediction_on_the_reference():
    """What the GPU test then shows on the device: on a linear unstable plant a stabilising LQR gain gives a smaller tr Sigma_H and a
    smaller chance-constraint value than the open loop."""
    from gaussian_process_mpc_amd.linearised import riccati_gain
    m = unstable_model()
    W = np.asarray(m["nominal"][0])
    K = riccati_gain(W[:, :2], W[:, 2:], np.eye(2), np.eye(1))
    assert np.abs(np.linalg.eigvals(W[:, :2] + W[:, 2:] @ K)).max() < 1.0 < np.abs(np.linalg.eigvals(W[:, :2])).max()
    x0, U = np.array([[0.1, -0.1]]), np.zeros((1, 6, 1))
    ol, cl = F.chain(m, x0, U, None), F.chain(m, x0, U, K)
    tr = lambda r: float(np.trace(f64(r["covs"][0, -1])))  # noqa: E731
    A, b, kap = np.array([[1.0, 0.0]]), np.array([0.5]), np.array([1.5])
    g_ol = f64(F.constraints(ol["means"], ol["covs"], None, A, b, kap)["g"])[0, -1, 0]
    g_cl = f64(F.constraints(cl["means"], cl["covs"], None, A, b, kap)["g"])[0, -1, 0]
    print("  tr Sigma_H: open loop %.4g, LQR %.4g; g: %.4g, %.4g" % (tr(ol), tr(cl), g_ol, g_cl))
    assert tr(cl) < 0.5 * tr(ol) and g_cl < g_ol


def unstable_model():
    """A two-state plant with an unstable linear nominal model and a small GP residual on top (also used by tests/test_gpu_linprop_fc.py)."""
    m = R.make_model(40, 2, 1, noise=True)
    m["beta"] = 0.02 * m["beta"]
    m["nominal"] = (np.array([[1.1, 0.3, 0.0], [0.0, 1.05, 0.5]]), np.zeros(2))
    return m


# ------------------------------------------------------------------------------------------------------------------ lqr
def test_riccati_gain_scalar_closed_form_and_two_states():
    from gaussian_process_mpc_amd.linearised import riccati_gain
    a, b, q, r = 1.2, 0.7, 2.0, 0.5
    # P = q + a^2 P - a^2 b^2 P^2 / (r + b^2 P)  <=>  b^2 P^2 + (r - a^2 r - q b^2) P - q r = 0, the positive root
    c1 = r - a * a * r - q * b * b
    Pr = (-c1 + np.sqrt(c1 * c1 + 4 * b * b * q * r)) / (2 * b * b)
    K = riccati_gain([[a]], [[b]], [[q]], [[r]])
    assert K.shape == (1, 1) and abs(K[0, 0] + a * b * Pr / (r + b * b * Pr)) <= 1e-12
    assert abs(a + b * K[0, 0]) < 1.0
    A, B = np.array([[1.1, 0.3], [0.0, 1.05]]), np.array([[0.0], [0.5]])
    Q, Rm = np.diag([1.0, 0.5]), np.array([[0.3]])
    K = riccati_gain(A, B, Q, Rm, iterations=2000)
    # recover P from the gain's own fixed point and check the Riccati equation
    P = Q.copy()
    for _ in range(2000):
        P = Q + A.T @ P @ A - A.T @ P @ B @ np.linalg.solve(Rm + B.T @ P @ B, B.T @ P @ A)
    resid = Q + A.T @ P @ A - A.T @ P @ B @ np.linalg.solve(Rm + B.T @ P @ B, B.T @ P @ A) - P
    assert np.abs(resid).max() <= 1e-10 * np.abs(P).max()
    assert np.abs(K + np.linalg.solve(Rm + B.T @ P @ B, B.T @ P @ A)).max() <= 1e-10
    assert np.abs(np.linalg.eigvals(A + B @ K)).max() < 1.0


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_abi_names_signatures_and_exports(L):
    from gaussian_process_mpc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    assert "Linearised propagation, full covariance" in hdr and "Hm_a[d][l]" in hdr and "P_ak P_bl + P_al P_bk" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        res, args = _lib.SIGNATURES[name]
        assert res in (ctypes.c_int, ctypes.c_size_t)
        assert getattr(L, name) is not None
        n_decl = len(re.search(r"\b%s\s*\((.*?)\);" % name, hdr, flags=re.S).group(1).split(","))
        assert n_decl == len(args), (name, n_decl, len(args))
    import gaussian_process_mpc_amd as g
    for name in ("linearised_step_full", "lqr_gain", "linearised_rollout", "mppi_solve_linearised"):
        assert hasattr(g, name) and name in g.__all__
    import inspect
    for fn in (g.linearised_rollout, g.mppi_solve_linearised):
        pr = inspect.signature(fn).parameters
        assert pr["full_covariance"].default is False and pr["feedback"].default is None
    assert hasattr(g.RiskSensitiveMPC, "set_feedback_gain") and hasattr(g.RiskSensitiveMPC, "clear_feedback_gain")


def _model_c(n=10, ds=2, da=1):
    from gaussian_process_mpc_amd._lib import GPModelC
    c = GPModelC()
    c.n, c.state_dim, c.action_dim = n, ds, da
    c.X = c.beta = c.Kinv = 0x1000                       # never dereferenced: every call below is refused before a launch
    c.ld, c.gp_stride = n, 0
    for k in range(ds * (ds + da)):
        c.lambdas[k] = 1.5
    for a in range(ds):
        c.sigma_f[a] = 1.0
    return c


def check_refusals(L):
    """Every refusal the header lists for the new entries: GPMPC_E_ARG with a text, and 0 from the size queries.  The pointers are not
    device memory: a call that got as far as a launch would fault or return GPMPC_E_LAUNCH, not GPMPC_E_ARG."""
    from gaussian_process_mpc_amd._lib import CostParamsC, StateConstraintsC
    p = ctypes.c_void_p
    a, b, c_, d, e = (p(0x2000 + 0x100 * i) for i in range(5))
    kk = p(0x8000)
    ws, big = p(0x9000), 1 << 40
    count = 0

    def refused(rc, what):
        nonlocal count
        assert rc == E_ARG, (what, rc)
        assert L.gpmpc_last_error().decode().startswith("gpmpc_linearised_fc"), (what, L.gpmpc_last_error())
        count += 1

    def step(m, B=4, mu=a, cov=b, U=c_, us=1, K=None, om=d, oc=e, jac=None, js=0, chunk=0, w=ws):
        return L.gpmpc_linearised_fc_step(ctypes.byref(m), B, mu, cov, U, us, K, om, oc, jac, js, chunk, w, big, None)

    def roll(m, B=4, H=3, x0=a, U=b, K=None, ks=0, cost=None, cons=None, flags=0, means=None, covs=None, jac=None, oc=None, og=None, g=None,
             gj=None, chunk=0, w=ws):
        return L.gpmpc_linearised_fc_rollout(ctypes.byref(m), B, H, x0, U, K, ks, None if cost is None else ctypes.byref(cost),
                                             None if cons is None else ctypes.byref(cons), flags, means, covs, jac, oc, og, g, gj, chunk, w, big,
                                             None)

    good = _model_c()
    # the model: what the diagonal entries refuse
    for field, value in (("state_dim", 0), ("state_dim", 9), ("action_dim", -1), ("action_dim", 7), ("n", 0), ("ld", 5), ("X", None),
                         ("beta", None), ("Kinv", None)):
        m = _model_c()
        setattr(m, field, value)
        refused(step(m), "step " + field)
        refused(roll(m), "rollout " + field)
    for arr, k, value in (("lambdas", 1, 0.0), ("lambdas", 2, float("inf")), ("sigma_f", 1, -1.0), ("sigma_f", 0, float("nan"))):
        m = _model_c()
        getattr(m, arr)[k] = value
        refused(step(m), "step " + arr)
        refused(roll(m), "rollout " + arr)
    m = _model_c()
    m.has_nominal, m.nom_w[1] = 1, float("nan")
    refused(step(m), "nominal")
    for arr, k, value in (("init_cov", 3, -1e-3), ("init_cov", 0, float("nan")), ("action_var", 0, -1.0), ("process_var", 1, float("inf"))):
        m = _model_c()
        m.has_noise = 1
        getattr(m, arr)[k] = value
        refused(step(m), "step " + arr)
        refused(roll(m), "rollout " + arr)
    # the whole init_cov: non-finite off the diagonal, asymmetric, a negative pivot
    for entries in ({0: 1e-3, 3: 1e-3, 1: float("nan"), 2: float("nan")}, {0: 1e-3, 3: 1e-3, 1: 5e-4, 2: 4e-4}, {0: 1e-3, 3: 1e-3, 1: 2e-3, 2: 2e-3}):
        m = _model_c()
        m.has_noise = 1
        for k, v in entries.items():
            m.init_cov[k] = v
        refused(step(m), "step init_cov %s" % entries)
        refused(roll(m), "rollout init_cov %s" % entries)
    # the step
    refused(step(good, B=0), "B")
    refused(step(good, chunk=-64), "chunk < 0")
    refused(step(good, chunk=100), "chunk % 64")
    for kw in (dict(mu=None), dict(cov=None), dict(U=None), dict(om=None), dict(oc=None), dict(w=None)):
        refused(step(good, **kw), "step NULL %s" % kw)
    refused(step(good, om=a), "aliasing")
    refused(step(good, us=0), "u_stride")
    refused(step(good, jac=p(0x7000), js=29), "jac_stride")                  # p (p + da) = 5 x 6 = 30
    noact = _model_c(da=0)
    refused(step(noact, U=None, K=kk), "a gain with da = 0")
    sz = L.gpmpc_linearised_fc_step_workspace_bytes
    assert sz(ctypes.byref(good), 0, 1, 0) == 0 and sz(ctypes.byref(good), 4, 1, 100) == 0
    assert sz(ctypes.byref(good), 4, 1, 0) > sz(ctypes.byref(good), 4, 0, 0) > 0
    assert L.gpmpc_linearised_fc_step(ctypes.byref(good), 4, a, b, c_, 1, None, d, e, None, 0, 0, ws, 16, None) == E_WORKSPACE
    # the rollout
    cost = CostParamsC()
    cost.Q[0] = cost.Q[3] = cost.R[0] = 1.0
    cons = StateConstraintsC()
    cons.n_rows, cons.A[0], cons.kappa[0] = 1, 1.0, 1.0
    refused(roll(good, B=0), "B")
    refused(roll(good, H=0), "H")
    refused(roll(good, chunk=32), "chunk")
    for flags in (4, 8, 16, 5, 2):
        refused(roll(good, flags=flags), "flags %d" % flags)
    refused(roll(good, x0=None), "x0")
    refused(roll(good, U=None), "U")
    refused(roll(good, w=None), "workspace")
    refused(roll(good, K=kk, ks=1), "k_step_stride 1")
    refused(roll(good, K=kk, ks=3), "k_step_stride 3")
    refused(roll(good, ks=5), "k_step_stride without a gain")
    refused(roll(noact, U=None, K=kk), "a gain with da = 0")
    refused(roll(good, jac=c_), "out_jac without WANT_GRAD")
    refused(roll(good, cost=cost), "cost without out_cost")
    refused(roll(good, cost=cost, oc=c_, flags=1), "cost + grad without out_grad")
    refused(roll(good, cons=cons), "cons without out_g")
    refused(roll(good, cons=cons, g=c_, flags=1), "cons + grad without out_gjac")
    bad_cons = StateConstraintsC()
    bad_cons.n_rows = 17
    refused(roll(good, cons=bad_cons, g=c_), "n_rows")
    bad_cons.n_rows, bad_cons.kappa[0] = 1, -1.0
    refused(roll(good, cons=bad_cons, g=c_), "kappa")
    sched = CostParamsC()
    sched.schedule_id = 987654
    rc = roll(good, cost=sched, oc=c_)
    assert rc == E_ARG and "cost schedule" in L.gpmpc_last_error().decode()
    refused(roll(noact, U=None, cost=cost, oc=c_), "cost with da = 0")
    refused(roll(good, B=1, H=64 * 65535 + 1), "H beyond the sweeps' grid")
    rz = L.gpmpc_linearised_fc_rollout_workspace_bytes
    assert rz(ctypes.byref(good), 4, 3, 4, 0) == 0 and rz(ctypes.byref(good), 4, 0, 0, 0) == 0
    assert rz(ctypes.byref(good), 1, 64 * 65535 + 1, 0, 0) == 0
    assert rz(ctypes.byref(good), 4, 3, 1, 0) > rz(ctypes.byref(good), 4, 3, 0, 0) > 0
    assert L.gpmpc_linearised_fc_rollout(ctypes.byref(good), 4, 3, a, b, None, 0, None, None, 0, None, None, None, None, None, None, None, 0, ws,
                                         16, None) == E_WORKSPACE
    # the pure functions
    vjp = lambda B=1, H=3, ds=2, da=1, jac=a, gU=b: L.gpmpc_linearised_fc_vjp(B, H, ds, da, jac, None, None, gU, None, None)  # noqa: E731
    for kw in (dict(jac=None), dict(gU=None), dict(B=0), dict(H=0), dict(ds=0), dict(ds=9), dict(da=0), dict(ds=5, da=4)):
        refused(vjp(**kw), "vjp %s" % kw)
    con = lambda B=1, H=3, ds=2, da=1, C=cons, mu=a, cv=b, jac=c_, g=d, gj=e: L.gpmpc_linearised_fc_constraints(  # noqa: E731
        B, H, ds, da, None if C is None else ctypes.byref(C), mu, cv, jac, g, gj, None)
    for kw in (dict(C=None), dict(mu=None), dict(cv=None), dict(g=None), dict(jac=None), dict(B=0), dict(H=0), dict(ds=9), dict(da=0),
               dict(C=bad_cons), dict(H=64 * 65535 + 1)):
        refused(con(**kw), "constraints %s" % kw)
    return count


def test_every_refusal_comes_before_a_launch(L):
    n = check_refusals(L)
    print("  %d refusals, each GPMPC_E_ARG with a text" % n)
    assert n >= 90
