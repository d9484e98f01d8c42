"""GPU tests of the linearised propagation against tests/linprop_reference.py (long double; include/gpmpc.h, "Linearised propagation").

Shapes are the smallest that cross every boundary of the kernels (csrc/linprop.hip: 64 x 64 tiles, 16-deep stages, GP groups, chunks):
    a   n = 70 (two row blocks, a ragged stage), ds = 2, da = 1, a lambda and a Kinv per GP, B = 3, H = 3
    b   n = 130 (three row blocks), ds = 3, da = 2, shared lambda and ONE Kinv (gp_stride = 0), B = 65 (two column tiles), H = 2
    c   n = 64, ds = 1, da = 1, B = 1 (padded columns)
    d   ds = 3 with the GPs 0 and 2 sharing (lambda, sf) and GP 1 apart, a nominal model, a non-default init_cov diagonal, action_var, process_var
    e   a Kinv made visibly non-symmetric (relative 1e-3 per entry)
    f   a sparse model (Z, alpha, Q) from SparseDynamics, M = 48

Bounds.  The project's budget: every sum is held to 1e-12 sum |terms| of the long double reference (tests/test_gpu_particles.py,
tests/test_gpu_gpstate.py), carried through the composite outputs by the formulas (linprop_reference.py: var' gets the budget of q plus
sum_d 2 |g_d| S_d times the budget of g_d, the Jacobian entries likewise); on var' and the Jacobian, not on the mean, plus 4 ulp of the
sizes the last few float64 additions round at (var' = ((sf^2 - q) + lin) + process_var and -dq + 2h are three roundings each).  Cost and gradient: the units of tests/cost_reference.py
(sums of the absolute terms, carried through the sweep over |J|), 1e-12 of them against the long double value, hence twice that between
two float64 routes."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import linprop_reference as R
import test_host_linprop as HT

pytestmark = pytest.mark.gpu
TOL = 1e-12
ULP = 2.0 ** -52
f64 = R.G.to_f64


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    return g


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


CASES = {"a": dict(n=70, ds=2, da=1, B=3, H=3), "b": dict(n=130, ds=3, da=2, kind="shared", B=65, H=2), "c": dict(n=64, ds=1, da=1, B=1, H=3),
         "d": dict(n=70, ds=3, da=1, pair=True, nominal=True, noise=True, B=3, H=3), "e": dict(n=70, ds=2, da=1, kind="nonsym", B=3, H=2)}


@functools.lru_cache(maxsize=None)
def case_model(name):
    kw = dict(CASES[name])
    kw.pop("B"), kw.pop("H")
    return R.make_model(kw.pop("n"), kw.pop("ds"), kw.pop("da"), **kw)


def device_model(G, m):
    ds, da, _ = R.dims(m)
    return G.GPModel(m["X"], m["beta"], m["Kinv"], m["lam"], m["sf"], ds, da, nominal=m.get("nominal"), init_cov=m.get("init_cov"),
                     action_var=m.get("action_var"), process_var=m.get("process_var"))


def worst_step(ref, mu, var, jac):
    """Worst |got - reference| / bound of the three outputs of a step."""
    bm = TOL * f64(ref["m_abs"])
    bv = TOL * f64(ref["var_abs"]) + 4 * ULP * f64(ref["var_mag"])
    bj = TOL * f64(ref["jac_abs"]) + 4 * ULP * f64(ref["jac_mag"])
    zero = bj == 0
    assert np.all(jac[zero] == 0.0)                                      # the structural zeros are written as zeros
    ej = np.abs(jac - f64(ref["jac"])) / np.where(zero, 1.0, bj)
    return float((np.abs(mu - f64(ref["mu"])) / bm).max()), float((np.abs(var - f64(ref["var"])) / bv).max()), float(ej.max())


def check_step(G, gm, m, B, label, control=None):
    mu, var, U = R.make_inputs(m, B)
    ref = R.step(m, mu, var, U)
    got = {}
    for chunk in (64, 0, 0):
        o = G.linearised_step(gm, mu, var, U, want_jac=True, chunk=chunk)
        got.setdefault(chunk, []).append(o)
    o64, o0, o0b = got[64][0], got[0][0], got[0][1]
    wm, wv, wj = worst_step(ref, *(t.cpu().numpy() for t in o0))
    print("  %s: mean %.3f, var %.3f, Jacobian %.3f of the bound" % (label, wm, wv, wj))
    assert wm <= 1.0 and wv <= 1.0 and wj <= 1.0
    assert all(same_bits(x, y) for x, y in zip(o64, o0)), "chunk = 64 differs from the default"
    assert all(same_bits(x, y) for x, y in zip(o0, o0b)), "two identical calls differ"
    nj = G.linearised_step(gm, mu, var, U, want_jac=False)                # without the Jacobian: the same mean and variance bits
    assert same_bits(nj[0], o0[0]) and same_bits(nj[1], o0[1])
    if control:
        miss = miss_against(R.step(m, mu, var, U, **{control: True}), ref, o0)
        print("  %s: the reference with %s misses by %.3g bounds" % (label, control, miss))
        assert miss >= 100.0
    return ref


def miss_against(bad, ref, o):
    """The device variance and Jacobian against a mistaken reference, in the bounds of the true one: the worst entry."""
    bv = TOL * f64(ref["var_abs"]) + 4 * ULP * f64(ref["var_mag"])
    bj = TOL * f64(ref["jac_abs"]) + 4 * ULP * f64(ref["jac_mag"])
    return max(float((np.abs(o[1].cpu().numpy() - f64(bad["var"])) / bv).max()),
               float((np.abs(o[2].cpu().numpy() - f64(bad["jac"])) / np.where(bj == 0, np.inf, bj)).max()))


# ------------------------------------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_step_against_reference(G, name):
    m = case_model(name)
    gm = device_model(G, m)
    if name == "b":
        assert gm.c.gp_stride == 0
    check_step(G, gm, m, CASES[name]["B"], "case " + name, control={"d": "drop_nominal_g", "a": "drop_h"}.get(name))


def test_step_nonsymmetric_inverse(G):
    """Values and Jacobians hold on an inverse perturbed by 1e-3 per entry; the "2 Kinv k" reference evaluated on the same input misses."""
    m = case_model("e")
    check_step(G, device_model(G, m), m, CASES["e"]["B"], "case e (non-symmetric Kinv)", control="r_twice")


def _sparse_dynamics(G):
    from gaussian_process_mpc_amd.synth import synth_problem
    pb = synth_problem(7, 200, 2, 1, 3, 2, sigma_n=0.05)
    idx = np.random.default_rng(5).choice(200, size=48, replace=False)
    dyn = G.SparseDynamics(2, 1, pb["X"][idx])
    for a, g in enumerate(dyn.gpr_err):
        g.set_lambdas(pb["lambdas"][a])
        g.set_sigma_f(0.9 + 0.3 * a)
        g.set_sigma_n(0.05)
    dyn.append_train_data(pb["X"][:, :2], pb["X"][:, 2:], pb["Y"])
    return dyn, pb


def test_step_sparse_model(G):
    dyn, pb = _sparse_dynamics(G)
    gm = G.GPModel.from_dynamics(dyn)
    assert gm.n == 48
    m = dict(X=gm.X.cpu().numpy(), beta=gm.beta.cpu().numpy(), Kinv=gm.Kinv.cpu().numpy(), lam=gm.lambdas, sf=gm.sigma_f)
    check_step(G, gm, m, 3, "case f (sparse, M = 48)")
    r = G.linearised_rollout(dyn, pb["x0"], pb["U"])                      # a SparseDynamics goes through GPModel.from_dynamics
    assert r["means"].shape == (2, 4, 2) and bool(torch.isfinite(r["vars"]).all())


# ------------------------------------------------------------------------------------------------------------------ the rollout
def cost_case(G, m, H, rng, schedule=False):
    """CostParams with a general Q, R, an input-rate weight and gamma != 0, next to the keyword arguments of cost_reference."""
    ds, da, _ = R.dims(m)
    Q = R.C.gen_Q(rng, ds)
    Rm, Rd = R.C.gen_R(rng, da), 0.3 * R.C.gen_R(rng, da)
    last_u, x_ref, u_ref = rng.uniform(-0.5, 0.5, da), rng.uniform(-0.5, 0.5, ds), rng.uniform(-0.5, 0.5, da)
    gamma = 0.7
    kw = dict(Rd=Rd, last_u=last_u, x_ref=x_ref, u_ref=u_ref)
    sched = None
    if schedule:
        X_ref, U_ref, Q_f = rng.uniform(-0.5, 0.5, (H + 1, ds)), rng.uniform(-0.5, 0.5, (H, da)), 2.0 * R.C.gen_Q(rng, ds)
        sched = G.CostSchedule(H, ds, da).set(X_ref, U_ref, Q_f)
        kw = dict(Rd=Rd, last_u=last_u, X_ref=X_ref, U_ref=U_ref, Q_f=Q_f)
    cp = G.CostParams(gamma, Q, Rm, R_delta=Rd, x_ref=x_ref, u_ref=u_ref, last_u=last_u, schedule=sched)
    return cp, (gamma, Q, Rm), kw


def device_cost_grad_vjp(G, cp, means, vars_, jac, U):
    """gpmpc_cost_grad on the diagonal covariances, then gpmpc_rollout_vjp fed with its local derivatives: (cost, grad)."""
    from gaussian_process_mpc_amd._lib import lib, ptr, stream_ptr, check
    B, H1, ds = means.shape
    H, da = H1 - 1, U.shape[2]
    covs = torch.diag_embed(vars_).contiguous()
    cost = torch.empty(B, dtype=torch.float64, device=means.device)
    dm, dc, du = torch.empty_like(means), torch.empty_like(covs), torch.empty_like(U)
    check(lib().gpmpc_cost_grad(B, H, ds, da, ctypes.byref(cp.c), ptr(means), ptr(covs), ptr(U), ptr(cost), ptr(dm), ptr(dc), ptr(du),
                                stream_ptr()), "gpmpc_cost_grad")
    dv = torch.diagonal(dc, dim1=2, dim2=3).contiguous()
    gU = torch.empty_like(U)
    check(lib().gpmpc_rollout_vjp(B, H, ds, da, ptr(jac), ptr(dm), ptr(dv), ptr(gU), None, stream_ptr()), "gpmpc_rollout_vjp")
    return cost, du + gU


@pytest.mark.parametrize("name,schedule", [("a", False), ("b", False), ("c", False), ("d", True)])
def test_rollout_chain_cost_gradient_constraints(G, name, schedule):
    from gaussian_process_mpc_amd.rollout import cost_full, rollout_constraints
    m = case_model(name)
    gm = device_model(G, m)
    ds, da, _ = R.dims(m)
    B, H = CASES[name]["B"], CASES[name]["H"]
    rng = np.random.default_rng(11)
    x0, U = rng.uniform(-1.0, 1.0, (B, ds)), rng.uniform(-1.0, 1.0, (B, H, da))
    cp, (gamma, Q, Rm), kw = cost_case(G, m, H, rng, schedule)
    sc = G.StateConstraints(rng.standard_normal((2, ds)), rng.uniform(0.0, 0.5, 2), kappa=[1.5, 0.0])
    r = G.linearised_rollout(gm, x0, U, cp, want_jac=True, constraints=sc)
    r2 = G.linearised_rollout(gm, x0, U, cp, want_jac=True, constraints=sc, chunk=64)
    for k in ("means", "vars", "jac", "cost", "grad", "g", "g_jac"):
        assert same_bits(r[k], r2[k]), k
    # the chain of step calls, bit for bit
    P0 = R.noise_model(m)[0]
    mu, var = torch.as_tensor(x0, device="cuda"), torch.as_tensor(np.broadcast_to(np.diag(P0), (B, ds)).copy(), device="cuda")
    assert same_bits(r["means"][:, 0], mu) and same_bits(r["vars"][:, 0], var)
    for t in range(H):
        mu, var, jac = G.linearised_step(gm, mu, var, U[:, t])
        assert same_bits(r["means"][:, t + 1], mu) and same_bits(r["vars"][:, t + 1], var) and same_bits(r["jac"][:, t], jac), t
    # objective only: the same bits without a Jacobian
    ro = G.linearised_rollout(gm, x0, U, cp, want_grad=False, constraints=sc)
    assert same_bits(ro["means"], r["means"]) and same_bits(ro["vars"], r["vars"]) and same_bits(ro["cost"], r["cost"]) and same_bits(ro["g"], r["g"])
    assert "grad" not in ro and "g_jac" not in ro
    # cost and gradient: the long double adjoint on the returned arrays; gpmpc_cost; gpmpc_cost_grad + gpmpc_rollout_vjp
    Ud = torch.as_tensor(U, device="cuda")
    ref = R.adjoint(r["jac"].cpu().numpy(), r["means"].cpu().numpy(), r["vars"].cpu().numpy(), U, gamma, Q, Rm, **kw)
    A_c, A_g = f64(ref["A_cost"]), f64(ref["A_grad"])
    c_full = cost_full(cp, r["means"], torch.diag_embed(r["vars"]).contiguous(), Ud).cpu().numpy()
    c_cg, g_vjp = device_cost_grad_vjp(G, cp, r["means"], r["vars"], r["jac"], Ud)
    cost, grad = r["cost"].cpu().numpy(), r["grad"].cpu().numpy()
    w = [np.abs(cost - f64(ref["cost"])) / (TOL * A_c), np.abs(grad - f64(ref["grad"])) / (TOL * A_g), np.abs(cost - c_full) / (2 * TOL * A_c),
         np.abs(cost - c_cg.cpu().numpy()) / (2 * TOL * A_c), np.abs(grad - g_vjp.cpu().numpy()) / (2 * TOL * A_g)]
    print("  case %s%s: cost %.3g, grad %.3g of the bound against the reference; cost vs gpmpc_cost %.3g, vs gpmpc_cost_grad %.3g, grad vs "
          "cost_grad + vjp %.3g" % ((name, " + schedule" if schedule else "") + tuple(float(x.max()) for x in w)))
    assert all(float(x.max()) <= 1.0 for x in w)
    # the whole chain in long double: the device trajectory stays within the budgets carried forward through |J| (first order, doubled)
    full = R.rollout(m, x0, U)
    err = np.zeros((B, 2 * ds))
    for t in range(H):
        s = R.step(m, f64(full["means"][:, t]), f64(full["vars"][:, t]), U[:, t])
        J = np.abs(f64(s["jac"]))[:, :, :2 * ds]
        tol_t = np.concatenate([TOL * f64(s["m_abs"]), TOL * f64(s["var_abs"]) + 4 * ULP * f64(s["var_mag"])], axis=1)
        err = np.einsum("brc,bc->br", J, err) + tol_t
        got = np.concatenate([r["means"][:, t + 1].cpu().numpy(), r["vars"][:, t + 1].cpu().numpy()], axis=1)
        want = np.concatenate([f64(full["means"][:, t + 1]), f64(full["vars"][:, t + 1])], axis=1)
        assert np.all(np.abs(got - want) <= 2.0 * err), t
    # constraints: what rollout_constraints gives on the returned arrays, bit for bit
    rc = rollout_constraints(r["means"], r["vars"], r["jac"], sc, ds, da)
    assert same_bits(rc["g"], r["g"]) and same_bits(rc["g_jac"], r["g_jac"])


# ------------------------------------------------------------------------------------------------------------------ MPPI
@pytest.mark.parametrize("constrained", [False, True])
def test_mppi_solve_linearised_is_the_host_loop(G, constrained):
    from gaussian_process_mpc_amd.mppi import mppi_sample, mppi_start, mppi_update
    m = case_model("a")
    gm = device_model(G, m)
    ds, da, H, K, iters = 2, 1, 4, 8, 3
    rng = np.random.default_rng(5)
    cp, _, _ = cost_case(G, m, H, rng)
    sc = G.StateConstraints(np.array([[1.0, 0.0]]), [0.3], kappa=1.0) if constrained else None
    x0, U0 = rng.uniform(-0.5, 0.5, ds), rng.uniform(-0.5, 0.5, (H, da))
    kw = dict(sigma=0.4, lb=-1.0, ub=1.0, seed=17, call_index=3)
    s = G.mppi_solve_linearised(gm, x0, U0, cp, constraints=sc, samples=K, iterations=iters, decay=0.8, beta=0.2, **kw)
    mean = torch.as_tensor(U0, device="cuda")
    best = mppi_start(mean)
    trace = []
    for it in range(iters):
        U, x0b = mppi_sample(mean, K, iteration=it, decay=0.8, x0=x0, **kw)
        r = G.linearised_rollout(gm, x0b, U, cp, want_grad=False, want_traj=False, constraints=sc)
        u = mppi_update(U, r["cost"], best, 0.2, g=r.get("g"), mean=mean)
        mean, best = u["mean"], u["best"]
        trace.append(u["trace"].cpu().numpy())
    b = best.cpu().numpy()
    assert np.array_equal(s["U"].reshape(-1), b[2:]) and s["violation"] == b[0] and s["cost"] == b[1]
    assert np.array_equal(s["trace"], np.stack(trace))
    assert np.isfinite(s["cost"])


# ------------------------------------------------------------------------------------------------------------------ RiskSensitiveMPC
def _mpc(G, H=5):
    from gaussian_process_mpc_amd.synth import synth_problem
    pb = synth_problem(3, 100, 2, 1, H, 4, sigma_n=0.05)
    mpc = G.RiskSensitiveMPC(0.5, H, 2, 1, pb["Q"], pb["R"])
    for a, g in enumerate(mpc.dynamics.gpr_err):
        g.set_lambdas(pb["lambdas"][a])
        g.set_sigma_f(0.8 + 0.3 * a)
        g.set_sigma_n(0.05)
    mpc.dynamics.append_train_data(pb["X"][:, :2], pb["X"][:, 2:], pb["Y"])
    mpc.train_empty = False
    mpc.curr_state = torch.as_tensor(pb["x0"][0], device=mpc.device).type(torch.float64)
    mpc.set_lb([-2.0]), mpc.set_ub([2.0])
    return mpc, pb


def test_mpc_linearised_callbacks_batch_and_default(G):
    mpc, pb = _mpc(G)
    H = mpc.horizon
    U = np.ascontiguousarray(pb["U"][:, :H])
    x = U[0].reshape(-1)
    # the default path: the bits of rollout called directly, with the attribute in place
    assert mpc.propagation == "moment_matching"
    direct = G.rollout(mpc.dynamics.pack(), mpc.curr_state, torch.as_tensor(U, device=mpc.device), mpc._cost_params(), want_grad=True)
    eb = mpc.evaluate_batch(U)
    for k in ("cost", "grad", "means", "vars"):
        assert same_bits(eb[k], direct[k]), k
    c_mm, g_mm = mpc.objective(x), np.array(mpc.gradient(x))
    cg = mpc.dynamics.pack().objective_gradient(pb["x0"][0], U[0], mpc._cost_params())
    assert c_mm == cg[0] and np.array_equal(g_mm.reshape(-1), cg[1:])
    # linearised: the four callbacks at one x are linearised_rollout at B = 1; evaluate_batch matches
    mpc.set_state_constraints(np.array([[1.0, 0.0]]), [0.4], prob=0.9)
    mpc.propagation = "linearised"
    r1 = G.linearised_rollout(mpc.dynamics, mpc.curr_state, U[:1], mpc._cost_params(), constraints=mpc.state_constraints)
    assert mpc.objective(x) == r1["cost"][0].item() and mpc.objective(x) != c_mm
    assert np.array_equal(np.asarray(mpc.gradient(x)), r1["grad"][0].cpu().numpy())
    assert np.array_equal(np.asarray(mpc.constraints(x)), r1["g"][0].cpu().numpy().reshape(-1))
    assert np.array_equal(np.asarray(mpc.jacobian(x)), r1["g_jac"][0].cpu().numpy().reshape(-1))
    rb = G.linearised_rollout(mpc.dynamics, mpc.curr_state, U, mpc._cost_params(), constraints=mpc.state_constraints)
    eb = mpc.evaluate_batch(U, constraints=True)
    for k in ("cost", "grad", "means", "vars", "g", "g_jac"):
        assert same_bits(eb[k], rb[k]), k
    assert same_bits(eb["cost"][:1], r1["cost"])                         # (columns are independent: B = 1 is the first column of the batch)
    # the solvers that take it: MPPI, and the host lock-step multi-start
    mpc.mppi_options.update(samples=16, iterations=3)
    plan = mpc.get_optimal_trajectory(pb["x0"][0], solver="mppi")
    assert plan.shape == (H, 1) and np.isfinite(mpc.last_solve_info["cost"]) and mpc.solver_used == "mppi x16"
    mpc.clear_state_constraints()
    mpc.multistart_options.update(max_ticks=3)
    plan = mpc.get_optimal_trajectory(pb["x0"][0], n_starts=2)
    assert plan.shape == (H, 1) and np.all(np.isfinite(plan)) and mpc.solver_used == "lockstep-lbfgs x2"
    # the refusals
    for solver in ("lbfgs", "auglag"):
        with pytest.raises(NotImplementedError, match="not yet"):
            mpc.get_optimal_trajectory(pb["x0"][0], solver=solver)
    mpc.full_covariance = True
    for call in (lambda: mpc.objective(x), lambda: mpc.evaluate_batch(U), lambda: mpc.get_optimal_trajectory(pb["x0"][0])):
        with pytest.raises(NotImplementedError, match="not yet"):
            call()
    mpc.full_covariance = False
    mpc.propagation = "taylor"
    with pytest.raises(ValueError, match="propagation"):
        mpc.objective(x)
    mpc.propagation = "moment_matching"
    assert mpc.objective(x) == c_mm


def test_validate_plan_third_column(G):
    mpc, pb = _mpc(G)
    U = pb["U"][0, :mpc.horizon]
    v0 = mpc.validate_plan(U=U, x0=pb["x0"][0], particles=1024, seed=0)
    v1 = mpc.validate_plan(U=U, x0=pb["x0"][0], particles=1024, seed=0, linearised=True)
    new = {"mean_lin", "var_lin", "z_mean_lin", "z_var_lin"}
    assert not (new & set(v0)) and set(v1) == set(v0) | new
    for k in v0:
        assert np.array_equal(np.asarray(v0[k]), np.asarray(v1[k])), k      # the other two columns are what they are without the argument
    for k in new:
        assert v1[k].shape == (mpc.horizon + 1, 2) and np.all(np.isfinite(v1[k])), k
    ln = G.linearised_rollout(mpc.dynamics, pb["x0"][0], U, None, want_grad=False)
    assert np.array_equal(v1["mean_lin"], ln["means"][0].cpu().numpy()) and np.array_equal(v1["var_lin"], ln["vars"][0].cpu().numpy())
    # step 1 starts from a point mass plus init_cov: the linearised mean is within a few standard errors of the particles there
    print("  validate_plan: step 1 z(mean) mm %s lin %s" % (np.round(v1["z_mean"][1], 2), np.round(v1["z_mean_lin"][1], 2)))


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_c_refusals_on_the_device(G):
    """Every refusal of the header, with a device present: GPMPC_E_ARG before a launch (the pointers handed over are not device memory)."""
    from gaussian_process_mpc_amd import _lib
    n = HT.check_refusals(_lib.lib())
    torch.cuda.synchronize()                                             # nothing was enqueued: no fault surfaces here
    assert n >= 75


def test_python_refusals(G):
    m = case_model("a")
    gm = device_model(G, m)
    mu, var, U = R.make_inputs(m, 3)
    with pytest.raises(G.GpmpcError, match="chunk"):
        G.linearised_step(gm, mu, var, U, chunk=100)
    with pytest.raises(ValueError, match="want_jac"):
        G.linearised_rollout(gm, mu, U[:, None, :], None, want_grad=False, want_jac=True)
    cp = G.CostParams(0.5, np.eye(3), np.eye(1))
    with pytest.raises(ValueError, match="shape mismatch"):
        G.linearised_rollout(gm, mu, U[:, None, :], cp)
    with pytest.raises(ValueError, match="constraint rows"):
        G.linearised_rollout(gm, mu, U[:, None, :], None, constraints=G.StateConstraints(np.ones((1, 3)), [0.0], kappa=0.0))
