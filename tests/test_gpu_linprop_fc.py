"""GPU tests of the full-covariance linearised propagation with state feedback against tests/linprop_fc_reference.py (long double;
include/gpmpc.h, "Linearised propagation, full covariance"; kernels in csrc/linprop_fc.hip).

Shapes: the CASES of tests/test_gpu_linprop.py, the smallest that cross every boundary of the tiling (two and three 64-row blocks, a ragged
stage, 65 columns, one padded column, GP groups with a gap, a nominal and a noise model, a visibly non-symmetric inverse, a sparse model).
Inputs: a non-diagonal SPD Sigma and a random gain of entries in [-0.5, 0.5].  Every check runs under the TILE and under the STREAM form
of stage A.

Bounds: the project's.  Every sum is held to 1e-12 sum |terms| of the long double reference, carried through the composite outputs by the
formulas in the reference's docstring, plus 4 ulp of the sizes the last float64 additions round at.  Cost and gradient: the units of
tests/cost_reference.py carried through the sweep over |J|, 1e-12 of them against the long double value, twice that between two float64
routes.  Structural zeros are exact zeros."""
import ctypes

import numpy as np
import pytest
import torch

import linprop_fc_reference as F
import linprop_reference as R
import test_gpu_linprop as TL
import test_host_linprop_fc as HF

pytestmark = pytest.mark.gpu
TOL, ULP, f64 = 1e-12, 2.0 ** -52, R.G.to_f64
CASES, case_model, device_model, same_bits = TL.CASES, TL.case_model, TL.device_model, TL.same_bits
FORMS = ["tile", "stream"]


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    return g


def bounds(ref):
    return (TOL * f64(ref["m_abs"]), TOL * f64(ref["cov_abs"]) + 4 * ULP * f64(ref["cov_mag"]),
            TOL * f64(ref["jac_abs"]) + 4 * ULP * f64(ref["jac_mag"]))


def worst_step(ref, mu, cov, jac):
    """Worst |got - reference| / bound of the three outputs of a step; the structural zeros are exact."""
    bm, bc, bj = bounds(ref)
    zero = bj == 0
    assert np.all(jac[zero] == 0.0)
    ej = np.abs(jac - f64(ref["jac"])) / np.where(zero, 1.0, bj)
    return float((np.abs(mu - f64(ref["mu"])) / bm).max()), float((np.abs(cov - f64(ref["cov"])) / bc).max()), float(ej.max())


def miss_against(bad, ref, o):
    """The device covariance and Jacobian against a mistaken reference, in the bounds of the true one: the worst entry."""
    _, bc, bj = bounds(ref)
    return max(float((np.abs(o[1].cpu().numpy() - f64(bad["cov"])) / bc).max()),
               float((np.abs(o[2].cpu().numpy() - f64(bad["jac"])) / np.where(bj == 0, np.inf, bj)).max()))


def check_step(G, gm, m, B, label, form, control=None, gain=True):
    mu, cov, U, K = F.make_inputs(m, B, gain=gain)
    ref = F.step(m, mu, cov, U, K)
    o64 = G.linearised_step_full(gm, mu, cov, U, K, chunk=64, form=form)
    o0 = G.linearised_step_full(gm, mu, cov, U, K, form=form)
    o0b = G.linearised_step_full(gm, mu, cov, U, K, form=form)
    wm, wc, wj = worst_step(ref, *(t.cpu().numpy() for t in o0))
    print("  %s [%s]: mean %.3f, Sigma' %.3f, Jacobian %.3f of the bound" % (label, form, wm, wc, wj))
    assert wm <= 1.0 and wc <= 1.0 and wj <= 1.0
    assert same_bits(o0[1], o0[1].transpose(1, 2).contiguous()), "Sigma' is not exactly symmetric"
    assert all(same_bits(x, y) for x, y in zip(o64, o0)), "chunk = 64 differs from the default"
    assert all(same_bits(x, y) for x, y in zip(o0, o0b)), "two identical calls differ"
    nj = G.linearised_step_full(gm, mu, cov, U, K, want_jac=False, form=form)
    assert same_bits(nj[0], o0[0]) and same_bits(nj[1], o0[1]), "mean / Sigma' differ without the Jacobian"
    diag = G.linearised_step(gm, mu, np.full(mu.shape, 1e-2), U, want_jac=False, form=form)
    assert same_bits(diag[0], o0[0]), "out_mu is not that of linearised_step"
    if control:
        miss = miss_against(F.step(m, mu, cov, U, K, **{control: True}), ref, o0)
        print("  %s [%s]: the reference with %s misses by %.3g bounds" % (label, form, control, miss))
        assert miss >= 100.0
    return ref


# ------------------------------------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_step_against_reference(G, name, form):
    m = case_model(name)
    gm = device_model(G, m)
    check_step(G, gm, m, CASES[name]["B"], "case " + name, form, control={"a": "drop_cross_hess", "d": "feedback_cross_dropped"}.get(name))


@pytest.mark.parametrize("form", FORMS)
def test_step_without_a_gain_and_sparse_model(G, form):
    m = case_model("a")
    check_step(G, device_model(G, m), m, 3, "case a, K = None", form, gain=False)
    dyn, pb = TL._sparse_dynamics(G)
    gm = G.GPModel.from_dynamics(dyn)
    assert gm.n == 48
    ms = dict(X=gm.X.cpu().numpy(), beta=gm.beta.cpu().numpy(), Kinv=gm.Kinv.cpu().numpy(), lam=gm.lambdas, sf=gm.sigma_f)
    check_step(G, gm, ms, 3, "case f (sparse, M = 48)", form)
    r = G.linearised_rollout(dyn, pb["x0"], pb["U"], full_covariance=True, form=form)   # a SparseDynamics goes through GPModel.from_dynamics
    assert r["means"].shape == (2, 4, 2) and r["covs"].shape == (2, 4, 2, 2) and bool(torch.isfinite(r["covs"]).all())


# ------------------------------------------------------------------------------------------------------------------ the rollout
def roll_model(name):
    """The case's model with a non-diagonal SPD init_cov (cases a and d; the others start from the default diagonal)."""
    m = dict(case_model(name))
    ds = R.dims(m)[0]
    if name in ("a", "d"):
        A = np.random.default_rng(4).standard_normal((ds, ds))
        P0 = 2e-3 * (A @ A.T) / ds + 1e-3 * np.eye(ds)
        m["init_cov"] = 0.5 * (P0 + P0.T)
    return m


def device_cost_grad_vjp(G, cp, means, covs, jac, U):
    """gpmpc_cost_grad on the full covariances, then gpmpc_linearised_fc_vjp fed with its local derivatives: (cost, grad)."""
    from gaussian_process_mpc_amd._lib import lib, ptr, stream_ptr, check
    B, H1, ds = means.shape
    H, da = H1 - 1, U.shape[2]
    cost = torch.empty(B, dtype=torch.float64, device=means.device)
    dm, dc, du = torch.empty_like(means), torch.empty_like(covs), torch.empty_like(U)
    check(lib().gpmpc_cost_grad(B, H, ds, da, ctypes.byref(cp.c), ptr(means), ptr(covs), ptr(U), ptr(cost), ptr(dm), ptr(dc), ptr(du),
                                stream_ptr()), "gpmpc_cost_grad")
    return cost, du + G.linearised_fc_vjp(jac, dm, dc, ds, da)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,schedule", [("a", False), ("b", False), ("c", False), ("d", True)])
def test_rollout_chain_cost_gradient_constraints(G, name, schedule, form):
    m = roll_model(name)
    gm = device_model(G, m)
    ds, da, _ = R.dims(m)
    B, H = CASES[name]["B"], CASES[name]["H"]
    rng = np.random.default_rng(11)
    x0, U = rng.uniform(-1.0, 1.0, (B, ds)), rng.uniform(-1.0, 1.0, (B, H, da))
    K = rng.uniform(-0.5, 0.5, (H, da, ds) if name in ("b", "d") else (da, ds))          # per-step gains on two cases, one gain on two
    cp, (gamma, Q, Rm), kw = TL.cost_case(G, m, H, rng, schedule)
    sc = G.StateConstraints(rng.standard_normal((2, ds)), rng.uniform(0.0, 0.5, 2), kappa=[1.5, 0.0])
    kwr = dict(want_jac=True, constraints=sc, full_covariance=True, feedback=K, form=form)
    r = G.linearised_rollout(gm, x0, U, cp, **kwr)
    r2 = G.linearised_rollout(gm, x0, U, cp, chunk=64, **kwr)
    for k in ("means", "covs", "jac", "cost", "grad", "g", "g_jac"):
        assert same_bits(r[k], r2[k]), k
    assert "vars" not in r
    # the chain of step calls, bit for bit
    P0 = R.noise_model(m)[0]
    mu, cov = torch.as_tensor(x0, device="cuda"), torch.as_tensor(np.broadcast_to(P0, (B, ds, ds)).copy(), device="cuda")
    assert same_bits(r["means"][:, 0], mu) and same_bits(r["covs"][:, 0], cov)
    for t in range(H):
        mu, cov, jac = G.linearised_step_full(gm, mu, cov, U[:, t], F.gain_at(K, t, ds, da), form=form)
        assert same_bits(r["means"][:, t + 1], mu) and same_bits(r["covs"][:, t + 1], cov) and same_bits(r["jac"][:, t], jac), t
    # objective only: the same bits without a Jacobian
    ro = G.linearised_rollout(gm, x0, U, cp, want_grad=False, constraints=sc, full_covariance=True, feedback=K, form=form)
    assert same_bits(ro["means"], r["means"]) and same_bits(ro["covs"], r["covs"]) and same_bits(ro["cost"], r["cost"]) and same_bits(ro["g"], r["g"])
    assert "grad" not in ro and "g_jac" not in ro
    # cost and gradient: the long double adjoint on the returned arrays; gpmpc_cost_grad + gpmpc_linearised_fc_vjp
    Ud = torch.as_tensor(U, device="cuda")
    means, covs, jacs = r["means"].cpu().numpy(), r["covs"].cpu().numpy(), r["jac"].cpu().numpy()
    ref = F.adjoint(jacs, means, covs, U, gamma, Q, Rm, **kw)
    A_c, A_g = f64(ref["A_cost"]), f64(ref["A_grad"])
    c_cg, g_vjp = device_cost_grad_vjp(G, cp, r["means"], r["covs"], r["jac"], Ud)
    cost, grad = r["cost"].cpu().numpy(), r["grad"].cpu().numpy()
    w = [np.abs(cost - f64(ref["cost"])) / (TOL * A_c), np.abs(grad - f64(ref["grad"])) / (TOL * A_g),
         np.abs(cost - c_cg.cpu().numpy()) / (2 * TOL * A_c), np.abs(grad - g_vjp.cpu().numpy()) / (2 * TOL * A_g)]
    print("  case %s%s [%s]: cost %.3g, grad %.3g of the bound against the reference; cost vs gpmpc_cost_grad %.3g, grad vs cost_grad + vjp "
          "%.3g" % ((name, " + schedule" if schedule else "", form) + tuple(float(x.max()) for x in w)))
    assert all(float(x.max()) <= 1.0 for x in w)
    # constraints: gpmpc_linearised_fc_constraints on the returned arrays, bit for bit; the reference sweep within its bound
    rc = G.linearised_fc_constraints(r["means"], r["covs"], r["jac"], sc, ds, da)
    assert same_bits(rc["g"], r["g"]) and same_bits(rc["g_jac"], r["g_jac"])
    cref = F.constraints(means, covs, jacs, sc.A, sc.b, sc.kappa)
    eg = np.abs(r["g"].cpu().numpy() - f64(cref["g"])) / (TOL * f64(cref["A_g"]))
    Aj = TOL * f64(cref["A_gjac"])
    gj = r["g_jac"].cpu().numpy()
    assert np.all(gj[Aj == 0] == 0.0)
    ej = np.abs(gj - f64(cref["gjac"])) / np.where(Aj == 0, 1.0, Aj)
    print("  case %s [%s]: constraints g %.3g, Jacobian %.3g of the bound" % (name, form, eg.max(), ej.max()))
    assert eg.max() <= 1.0 and ej.max() <= 1.0
    m_c = sc.m
    for t in range(1, H + 1):                                # causality: exact zeros, sign included
        blk = gj[:, (t - 1) * m_c:t * m_c, t * da:]
        assert not np.any(blk) and not np.any(np.signbit(blk)), t
    # the whole chain in long double: the device trajectory stays within the step budgets carried forward through |J| (first order, doubled)
    full = F.chain(m, x0, U, K)
    p = F.packed_dim(ds)
    err = np.zeros((B, p))
    for t in range(H):
        s = full["steps"][t]
        bm, bc, _ = bounds(s)
        tol_t = f64(F.pack_state(bm, bc))
        err = np.einsum("brc,bc->br", np.abs(f64(s["jac"]))[:, :, :p], err) + tol_t
        got = F.pack_state(means[:, t + 1], covs[:, t + 1])
        want = f64(F.pack_state(full["means"][:, t + 1], full["covs"][:, t + 1]))
        assert np.all(np.abs(got - want) <= 2.0 * err), t


@pytest.mark.parametrize("form", FORMS)
def test_open_loop_diagonal_start_meets_the_diagonal_rollout(G, form):
    """K = None from a diagonal init_cov: step 1's diagonal is the diagonal rollout's vars[:, 1], within the sum of the two bounds."""
    m = case_model("d")
    gm = device_model(G, m)
    ds, da, _ = R.dims(m)
    rng = np.random.default_rng(2)
    x0, U = rng.uniform(-1.0, 1.0, (3, ds)), rng.uniform(-1.0, 1.0, (3, 2, da))
    rf = G.linearised_rollout(gm, x0, U, full_covariance=True, want_grad=False, form=form)
    rd = G.linearised_rollout(gm, x0, U, want_grad=False, form=form)
    assert same_bits(rf["means"][:, 1], rd["means"][:, 1])
    P0 = R.noise_model(m)[0]
    dref = R.step(m, x0, np.broadcast_to(np.diag(P0), (3, ds)), U[:, 0])
    fref = F.step(m, x0, np.broadcast_to(P0, (3, ds, ds)), U[:, 0], None)
    bd = TOL * f64(dref["var_abs"]) + 4 * ULP * f64(dref["var_mag"])
    bf = np.stack([bounds(fref)[1][:, k, k] for k in range(ds)], axis=1)
    e = np.abs(torch.diagonal(rf["covs"][:, 1], dim1=1, dim2=2).cpu().numpy() - rd["vars"][:, 1].cpu().numpy()) / (bd + bf)
    print("  [%s] step 1 diagonal vs the diagonal rule: %.3g of the two bounds" % (form, e.max()))
    assert e.max() <= 1.0


# ------------------------------------------------------------------------------------------------------------------ feedback, MPC
def test_lqr_gain_and_feedback_shrink_the_prediction(G):
    """On the plant where the reference shows it on the CPU (tests/test_host_linprop_fc.py): lqr_gain reads A, B from the device step, the
    closed loop it makes is stable, and tr Sigma_H and a chance-constraint value come out smaller than with no gain."""
    m = HF.unstable_model()
    gm = device_model(G, m)
    W = np.asarray(m["nominal"][0])
    K = G.lqr_gain(gm, np.zeros(2), np.zeros(1), np.eye(2), np.eye(1))
    assert K.shape == (1, 2)
    jac = G.linearised_step(gm, np.zeros((1, 2)), np.zeros((1, 2)), np.zeros((1, 1)))[2][0].cpu().numpy()
    A, Bm = jac[:2, :2], jac[:2, 4:]
    assert np.abs(A - W[:, :2]).max() < 0.1 and np.abs(np.linalg.eigvals(A)).max() > 1.0 > np.abs(np.linalg.eigvals(A + Bm @ K)).max()
    x0, U = np.array([[0.1, -0.1]]), np.zeros((1, 6, 1))
    sc = G.StateConstraints(np.array([[1.0, 0.0]]), [0.5], kappa=1.5)
    ol = G.linearised_rollout(gm, x0, U, constraints=sc, full_covariance=True, want_grad=False)
    cl = G.linearised_rollout(gm, x0, U, constraints=sc, feedback=K, want_grad=False)
    tr = lambda r: float(torch.diagonal(r["covs"][0, -1]).sum().item())  # noqa: E731
    print("  tr Sigma_H: open loop %.4g, LQR %.4g; g_H: %.4g, %.4g" % (tr(ol), tr(cl), ol["g"][0, -1, 0].item(), cl["g"][0, -1, 0].item()))
    assert tr(cl) < 0.5 * tr(ol) and cl["g"][0, -1, 0].item() < ol["g"][0, -1, 0].item()
    # a nominal-only scalar plant: the gain is the closed-form Riccati root's
    n1 = R.make_model(20, 1, 1)
    n1["beta"] = np.zeros_like(n1["beta"])
    a, b, q, r = 1.2, 0.7, 2.0, 0.5
    n1["nominal"] = (np.array([[a, b]]), np.zeros(1))
    K1 = G.lqr_gain(device_model(G, n1), [0.3], [0.1], [[q]], [[r]])
    c1 = r - a * a * r - q * b * b
    Pr = (-c1 + np.sqrt(c1 * c1 + 4 * b * b * q * r)) / (2 * b * b)
    assert abs(K1[0, 0] + a * b * Pr / (r + b * b * Pr)) <= 1e-12


def test_mpc_linearised_full(G):
    """propagation = "linearised_full": the callbacks are linearised_rollout(..., full_covariance=True, feedback=K) at B = 1; the objective's
    central differences bracket the analytic gradient; MPPI with constraints and the host multi-start return plans; the refusals.

    The bracket: central differences along a direction at relative steps 1e-4 ... 1e-7 carry a truncation error that falls with h^2 and a
    rounding error that grows with 1 / h, so over three decades they scatter around the derivative by no more than they differ among
    themselves: the analytic directional derivative has to lie in their hull widened by its own width on either side."""
    mpc, pb = TL._mpc(G)
    H = mpc.horizon
    U = np.ascontiguousarray(pb["U"][:, :H])
    x = U[0].reshape(-1)
    mpc.set_state_constraints(np.array([[1.0, 0.0]]), [0.4], prob=0.9)
    mpc.propagation = "linearised"
    c_diag = mpc.objective(x)
    mpc.propagation = "linearised_full"
    mpc.full_covariance = True                                               # not consulted under this rule
    K = G.lqr_gain(mpc.dynamics, pb["x0"][0], U[0, 0], np.eye(2), np.eye(1))
    c_open = mpc.objective(x)
    mpc.set_feedback_gain(K)
    r1 = G.linearised_rollout(mpc.dynamics, mpc.curr_state, U[:1], mpc._cost_params(), constraints=mpc.state_constraints, full_covariance=True,
                              feedback=K)
    c, g = mpc.objective(x), np.asarray(mpc.gradient(x))
    assert np.isfinite(c) and np.all(np.isfinite(g)) and c == r1["cost"][0].item() and c != c_open and c_open != c_diag
    assert np.array_equal(g, r1["grad"][0].cpu().numpy())
    assert np.array_equal(np.asarray(mpc.constraints(x)), r1["g"][0].cpu().numpy().reshape(-1))
    assert np.array_equal(np.asarray(mpc.jacobian(x)), r1["g_jac"][0].cpu().numpy().reshape(-1))
    eb = mpc.evaluate_batch(U, constraints=True)
    rb = G.linearised_rollout(mpc.dynamics, mpc.curr_state, U, mpc._cost_params(), constraints=mpc.state_constraints, feedback=K)
    for k in ("cost", "grad", "means", "covs", "g", "g_jac"):
        assert same_bits(eb[k], rb[k]), k
    assert same_bits(eb["cost"][:1], r1["cost"])
    # central differences of the objective (and of the first constraint row) bracket the analytic derivative
    v = np.random.default_rng(1).standard_normal(x.size)
    v /= np.linalg.norm(v)
    scale = max(1.0, float(np.abs(x).max()))
    for what, f, an in (("objective", lambda y: mpc.objective(y), float(g.reshape(-1) @ v)),
                        ("constraint g[H]", lambda y: float(np.asarray(mpc.constraints(y))[-1]),
                         float(np.asarray(mpc.jacobian(x)).reshape(H, -1)[-1] @ v))):
        fd = [(f(x + h * scale * v) - f(x - h * scale * v)) / (2 * h * scale) for h in (1e-4, 1e-5, 1e-6, 1e-7)]
        lo, hi = min(fd), max(fd)
        print("  %s: analytic %.12g, central differences %s" % (what, an, ", ".join("%.12g" % d for d in fd)))
        assert lo - (hi - lo) <= an <= hi + (hi - lo), (what, an, fd)
    # the solvers that take it
    mpc.mppi_options.update(samples=16, iterations=3)
    plan = mpc.get_optimal_trajectory(pb["x0"][0], solver="mppi")
    assert plan.shape == (H, 1) and np.all(np.isfinite(plan)) and np.isfinite(mpc.last_solve_info["cost"]) and mpc.solver_used == "mppi x16"
    mpc.clear_state_constraints()
    plan = mpc.get_optimal_trajectory(pb["x0"][0], solver="mppi")
    assert plan.shape == (H, 1) and np.all(np.isfinite(plan))
    mpc.multistart_options.update(max_ticks=3)
    plan = mpc.get_optimal_trajectory(pb["x0"][0], n_starts=2)
    assert plan.shape == (H, 1) and np.all(np.isfinite(plan)) and mpc.solver_used == "lockstep-lbfgs x2"
    # the refusals
    for solver in ("lbfgs", "auglag"):
        with pytest.raises(NotImplementedError, match="not yet"):
            mpc.get_optimal_trajectory(pb["x0"][0], solver=solver)
    for prop in ("linearised", "moment_matching"):
        mpc.propagation = prop
        mpc.full_covariance = False
        with pytest.raises(ValueError, match="feedback gain"):
            mpc.objective(x)
    mpc.clear_feedback_gain()
    mpc.propagation, mpc.full_covariance = "linearised", True
    with pytest.raises(NotImplementedError, match="not yet"):
        mpc.objective(x)
    mpc.full_covariance = False
    assert mpc.objective(x) == c_diag
    with pytest.raises(ValueError, match="feedback gain"):
        mpc.set_feedback_gain(np.zeros((3, 3)))


def test_mppi_host_loop_matches_its_parts(G):
    from gaussian_process_mpc_amd.mppi import mppi_sample, mppi_start, mppi_update
    m = case_model("a")
    gm = device_model(G, m)
    ds, da, H, Ks, iters = 2, 1, 4, 8, 2
    rng = np.random.default_rng(5)
    cp, _, _ = TL.cost_case(G, m, H, rng)
    sc = G.StateConstraints(np.array([[1.0, 0.0]]), [0.3], kappa=1.0)
    x0, U0, K = rng.uniform(-0.5, 0.5, ds), rng.uniform(-0.5, 0.5, (H, da)), rng.uniform(-0.5, 0.5, (da, ds))
    kw = dict(sigma=0.4, lb=-1.0, ub=1.0, seed=17, call_index=3)
    s = G.mppi_solve_linearised(gm, x0, U0, cp, constraints=sc, samples=Ks, iterations=iters, decay=0.8, beta=0.2, feedback=K, **kw)
    mean = torch.as_tensor(U0, device="cuda")
    best = mppi_start(mean)
    for it in range(iters):
        U, x0b = mppi_sample(mean, Ks, iteration=it, decay=0.8, x0=x0, **kw)
        r = G.linearised_rollout(gm, x0b, U, cp, want_grad=False, want_traj=False, constraints=sc, feedback=K)
        u = mppi_update(U, r["cost"], best, 0.2, g=r.get("g"), mean=mean)
        mean, best = u["mean"], u["best"]
    b = best.cpu().numpy()
    assert np.array_equal(s["U"].reshape(-1), b[2:]) and s["violation"] == b[0] and s["cost"] == b[1] and np.isfinite(s["cost"])
    assert s["trace"].shape == (iters, 6)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_c_refusals_on_the_device(G):
    """Every refusal of the header, with a device present: GPMPC_E_ARG before a launch (the pointers handed over are not device memory)."""
    from gaussian_process_mpc_amd import _lib
    n = HF.check_refusals(_lib.lib())
    torch.cuda.synchronize()                                             # nothing was enqueued: no fault surfaces here
    assert n >= 90


def test_python_refusals(G):
    m = case_model("a")
    gm = device_model(G, m)
    mu, cov, U, K = F.make_inputs(m, 3)
    with pytest.raises(G.GpmpcError, match="chunk"):
        G.linearised_step_full(gm, mu, cov, U, K, chunk=100)
    with pytest.raises(ValueError, match="feedback gain"):
        G.linearised_step_full(gm, mu, cov, U, np.zeros((2, 2)))
    with pytest.raises(ValueError, match="feedback gain"):
        G.linearised_rollout(gm, mu, U[:, None, :], None, feedback=np.zeros((3, 1, 2)))
    with pytest.raises(ValueError, match="want_jac"):
        G.linearised_rollout(gm, mu, U[:, None, :], None, want_grad=False, want_jac=True, full_covariance=True)
