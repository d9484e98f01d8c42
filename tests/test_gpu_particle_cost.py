"""GPU tests of the particle cost (include/gpmpc.h, "Particle cost"; csrc/particle_cost.hip) against tests/particle_cost_reference.py
(long double).

Rounding budgets, in the project's convention (1e-12 x the sum of absolute terms, a function of the reference alone):

  stage, gamma == 0    1e-12 (1 / P) sum_p c_abs_p, c_abs_p = sum_kl |e_k| |Q_kl| |e_l|: every c_p is within that of its value, and the sum of
                       non-negative-budget terms adds P / 256 + 8 roundings of at most |c_p| <= c_abs_p each.
  stage, gamma != 0    s = -(2 / gamma) (logsumexp(a) - log P), a_p = -(gamma / 2) c_p.  logsumexp is 1-Lipschitz in the sup norm, so the
                       error of the a_p (quadratic form, the product with gamma / 2) reaches s as at most max_p of it times 2 / |gamma|:
                       1e-12 max_p c_abs_p.  The value itself is three roundings of |s| <= max_p |c_p| (the sum M + log, 2 / gamma, the
                       product), far inside the same term.  What is left is the conditioning term (2 / |gamma|) k ULP, the relative
                       error of S = sum_p exp(a_p - M) in [1, P] and the absolute error of its logarithm, counted in roundings of 2^-53
                       by operation: the subtraction a_p - M weighted by exp(a_p - M) (x e^-x <= 1 / e: 1), exp (2), the thread's
                       sum of up to 16 terms (16), the fold of 256 partial sums (8), the division by P (1), log (1 relative to
                       |log(S / P)| <= log 4096 = 8.4: 9): 37; k = 40 with ULP = 2^-52 leaves a factor two.
  cost                 the stage budgets, plus 1e-12 (sum_i |s_i| + the absolute input terms of cost_reference.input_terms).
  g                    1e-12 (max_p sum_k |a_rk x_k| + |b_r|): every margin is within that of its value, and an order statistic is
                       1-Lipschitz in the sup norm of the margins.

Shapes: P in {1, 2, 63, 64, 257, 300, 4096} (one particle, below and above a wave, two per thread, a sort that is no power of two, the
cap), three (ds, da), B = 3, H = 3: every case is one launch pair and a long double reference of at most 4 x 3 x 4096 particles."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cost_reference as CR
import mppi_reference as MR
import particle_cost_reference as PC

pytestmark = pytest.mark.gpu
TOL = 1e-12
ULP = 2.0 ** -52
K_OPS = 40.0
B, H = 3, 3
GAMMAS = (0.0, 1e-5, 0.7, -0.4)


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    return g


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------ 1. the pure kernel
@functools.lru_cache(maxsize=None)
def synthetic(ds, da, P, variant="plain"):
    """Particles (H+1, B, P, ds) spread around a per-plan, per-step centre, plans U, a cost and constraint rows.  variant: plain (symmetric
    Q, three rows) | nonsym_Q | schedule (rows X_ref / U_ref and a terminal weight) | R_delta | rows1 | rows16 | ties (every particle
    value appears at least twice, a third of them eight times)."""
    rng = np.random.default_rng([ds, da, P, sum(map(ord, variant))])
    X = rng.uniform(-0.8, 0.8, (H + 1, B, 1, ds)) + 0.35 * rng.standard_normal((H + 1, B, P, ds))
    if variant == "ties":
        X[:, :, 1::2] = X[:, :, 0:2 * (P // 2):2]
        X[:, :, :P // 3] = X[:, :, (np.arange(P // 3) // 8) * 8]
    U = rng.uniform(-1.0, 1.0, (B, H, da))
    A = rng.standard_normal((ds, ds))
    kw = dict(Q=A @ A.T / ds + 0.3 * np.eye(ds), R=CR.gen_R(rng, da), x_ref=rng.uniform(-0.3, 0.3, ds), u_ref=rng.uniform(-0.3, 0.3, da))
    if variant == "nonsym_Q":
        kw["Q"] = CR.gen_Q(rng, ds)
    if variant == "schedule":
        kw.update(X_ref=rng.uniform(-0.5, 0.5, (H + 1, ds)), U_ref=rng.uniform(-0.5, 0.5, (H, da)), Q_f=CR.gen_Q(rng, ds))
    if variant == "R_delta":
        kw.update(Rd=CR.gen_R(rng, da), last_u=rng.uniform(-0.5, 0.5, da))
    m = {"rows1": 1, "rows16": 16}.get(variant, 3)
    rows = (rng.standard_normal((m, ds)), rng.uniform(-0.3, 0.6, m), np.array([0.0, 1.0, 2.3, 0.4, 1.645, 3.0, 0.1, 0.8] * 2)[:m])
    return dict(X=X, U=U, kw=kw, rows=rows, ds=ds, da=da, P=P)


def device_cost(G, pb, gamma):
    kw = pb["kw"]
    sched = None
    if "X_ref" in kw:
        sched = G.CostSchedule(H, pb["ds"], pb["da"])
        sched.set(kw["X_ref"], kw["U_ref"], kw["Q_f"])            # (the parameters keep it alive)
    return G.CostParams(gamma, kw["Q"], kw["R"], R_delta=kw.get("Rd"), x_ref=kw["x_ref"], u_ref=kw["u_ref"], last_u=kw.get("last_u"), schedule=sched)


def budgets(ref, gamma, P):
    ca = f64(ref["c_abs"])
    stage = TOL * ca.mean(axis=2) if gamma == 0.0 else TOL * ca.max(axis=2) + (2.0 / abs(gamma)) * K_OPS * ULP
    cost = stage.sum(axis=1) + TOL * (np.abs(f64(ref["stage"])).sum(axis=1) + f64(ref["A_input"]))
    return stage, cost, TOL * f64(ref["g_unit"])


def run_case(G, pb, gamma):
    """The device against the reference on one problem: the worst fraction of each budget."""
    sc = G.StateConstraints(pb["rows"][0], pb["rows"][1], kappa=pb["rows"][2])
    Xd = torch.as_tensor(pb["X"], device="cuda")
    got = G.particle_cost(Xd, pb["U"], device_cost(G, pb, gamma), constraints=sc)
    ref = PC.cost(pb["X"], pb["U"], gamma=gamma, cons=pb["rows"], **pb["kw"])
    bs, bc, bg = budgets(ref, gamma, pb["P"])
    ws = float((np.abs(got["stage"].cpu().numpy() - f64(ref["stage"])) / bs).max())
    wc = float((np.abs(got["cost"].cpu().numpy() - f64(ref["cost"])) / bc).max())
    wg = float((np.abs(got["g"].cpu().numpy() - f64(ref["g"])) / bg).max())
    return ws, wc, wg, got, ref, (bs, bc, bg)


@pytest.mark.parametrize("P", [1, 2, 63, 64, 257, 300, 4096])
@pytest.mark.parametrize("dims", [(1, 1), (3, 2), (4, 1)], ids=lambda d: "ds%d_da%d" % d)
def test_particle_cost_grid(G, dims, P):
    pb = synthetic(dims[0], dims[1], P)
    for gamma in GAMMAS:
        ws, wc, wg, _, _, _ = run_case(G, pb, gamma)
        print("  ds %d da %d P %4d gamma %+.0e: stage %.3f, cost %.3f, g %.3f of the budget" % (dims[0], dims[1], P, gamma, ws, wc, wg))
        assert ws <= 1.0 and wc <= 1.0 and wg <= 1.0


@pytest.mark.parametrize("variant", ["nonsym_Q", "schedule", "R_delta", "rows1", "rows16", "ties"])
def test_particle_cost_variants(G, variant):
    pb = synthetic(3, 2, 300, variant)
    for gamma in GAMMAS:
        ws, wc, wg, got, ref, _ = run_case(G, pb, gamma)
        print("  %-9s gamma %+.0e: stage %.3f, cost %.3f, g %.3f of the budget" % (variant, gamma, ws, wc, wg))
        assert ws <= 1.0 and wc <= 1.0 and wg <= 1.0
        assert got["g"].shape == (B, H, pb["rows"][0].shape[0])


def test_input_terms_are_those_of_gpmpc_cost_bit_for_bit(G):
    """Every particle AT the reference and gamma = 0: all stage costs are exactly 0 and J is the input cost alone -- the bits gpmpc_cost
    returns for means at the reference and zero covariances, with u_ref, R_delta / last_u and the rows of a schedule."""
    from gaussian_process_mpc_amd.rollout import cost_full
    for variant in ("plain", "R_delta", "schedule"):
        pb = synthetic(3, 2, 64, variant)
        cost = device_cost(G, pb, 0.0)
        xr = pb["kw"].get("X_ref", np.tile(pb["kw"]["x_ref"], (H + 1, 1)))
        X = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(xr[:, None, None, :], (H + 1, B, 64, 3))), device="cuda")
        got = G.particle_cost(X, pb["U"], cost)
        means = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(xr[None], (B, H + 1, 3))), device="cuda")
        want = cost_full(cost, means, torch.zeros(B, H + 1, 3, 3, dtype=torch.float64, device="cuda"), torch.as_tensor(pb["U"], device="cuda"))
        assert bool((got["stage"] == 0.0).all()) and torch.equal(got["cost"], want), variant
        assert float(want.abs().min().item()) > 0.0


def test_cost_without_a_stage_buffer_is_the_same_bits(G):
    from gaussian_process_mpc_amd._lib import lib, ptr, stream_ptr
    for variant, gamma in (("plain", 0.7), ("schedule", -0.4), ("R_delta", 0.0)):
        pb = synthetic(3, 2, 300, variant)
        cost = device_cost(G, pb, gamma)
        sc = G.StateConstraints(pb["rows"][0], pb["rows"][1], kappa=pb["rows"][2])
        X, U = torch.as_tensor(pb["X"], device="cuda"), torch.as_tensor(pb["U"], device="cuda")
        with_stage = G.particle_cost(X, U, cost, constraints=sc)
        out, g = torch.empty(B, dtype=torch.float64, device="cuda"), torch.empty(B, H, 3, dtype=torch.float64, device="cuda")
        rc = lib().gpmpc_particle_cost(B, 300, H, 3, 2, ctypes.byref(cost.c), ctypes.byref(sc.c), ptr(X), ptr(U), ptr(out), None, ptr(g), stream_ptr())
        assert rc == 0 and torch.equal(out, with_stage["cost"]) and torch.equal(g, with_stage["g"]), variant


def test_controls_miss_on_the_device_inputs(G):
    """The three mistakes of tests/test_host_particle_cost.py against what the DEVICE returns: each misses the budget by a wide factor."""
    pb = synthetic(3, 2, 300)
    ws, wc, wg, got, ref, (bs, bc, bg) = run_case(G, pb, 0.7)
    assert max(ws, wc, wg) <= 1.0
    stage, g = got["stage"].cpu().numpy(), got["g"].cpu().numpy()
    for name, wrong in (("gamma with the wrong sign", dict(gamma_sign=-1.0)), ("the mean in the place of the entropic risk", dict(mean_only=True))):
        bad = PC.cost(pb["X"], pb["U"], gamma=0.7, cons=pb["rows"], **pb["kw"], **wrong)
        miss = float((np.abs(stage - f64(bad["stage"])) / bs).min())
        print("  control %s: misses by at least %.3g budgets" % (name, miss))
        assert miss > 1e3
    for shift in (-1, 1):
        bad = PC.cost(pb["X"], pb["U"], gamma=0.7, cons=pb["rows"], index_shift=shift, **pb["kw"])
        miss = float(np.median(np.abs(g - f64(bad["g"])) / bg))
        print("  control index P - m %+d: misses by %.3g budgets (median)" % (shift, miss))
        assert miss > 1e3


# ------------------------------------------------------------------------------------------------------------------ 2. NaN
def test_nan_particle_poisons_its_plan_and_step_only(G):
    pb = synthetic(3, 2, 300)
    sc = G.StateConstraints(pb["rows"][0], pb["rows"][1], kappa=pb["rows"][2])
    for gamma in (0.0, 0.7):
        cost = device_cost(G, pb, gamma)
        clean = G.particle_cost(torch.as_tensor(pb["X"], device="cuda"), pb["U"], cost, constraints=sc)
        X = pb["X"].copy()
        X[2, 1, 277, 1] = np.nan
        got = G.particle_cost(torch.as_tensor(X, device="cuda"), pb["U"], cost, constraints=sc)
        want_stage, want_g = torch.zeros(B, H + 1, dtype=torch.bool, device="cuda"), torch.zeros(B, H, 3, dtype=torch.bool, device="cuda")
        want_stage[1, 2], want_g[1, 1, :] = True, True
        assert torch.equal(torch.isnan(got["stage"]), want_stage) and torch.equal(torch.isnan(got["g"]), want_g)
        assert torch.isnan(got["cost"]).cpu().tolist() == [False, True, False]
        assert torch.equal(got["stage"][~want_stage], clean["stage"][~want_stage]) and torch.equal(got["g"][~want_g], clean["g"][~want_g])
        assert torch.equal(got["cost"][[0, 2]], clean["cost"][[0, 2]])


# ------------------------------------------------------------------------------------------------------------------ 3. streaming = stored
HS, SEED, CALL = 4, 11, 2


def _stream_model(G, kind):
    import test_gpu_particles as TP
    if kind == "sparse":
        return G.GPModel.from_dynamics(TP._dynamics(G, "sparse")[0])
    m = TP.model_data(70, 2, 1, "pergp") if kind == "dense" else TP.model_data(70, 2, 1, "shared", process_var=True, nominal=True)
    return TP.device_model(G, m)


@pytest.mark.parametrize("P", [35, 300])
@pytest.mark.parametrize("kind", ["dense", "sparse", "nominal_noise"])
def test_evaluate_is_the_cost_of_the_stored_rollout_bit_for_bit(G, kind, P):
    gm = _stream_model(G, kind)
    rng = np.random.default_rng(17)
    x0, U = rng.uniform(-0.6, 0.6, (B, 2)), rng.uniform(-0.8, 0.8, (B, HS, 1))
    cost = G.CostParams(0.7, np.array([[1.0, 0.2], [0.1, 0.6]]), np.array([[0.3]]), R_delta=np.array([[0.05]]), x_ref=[0.1, -0.1], u_ref=[0.05], last_u=[0.2])
    sc = G.StateConstraints(np.array([[1.0, 0.0], [0.3, -0.8]]), [0.4, 0.2], kappa=[0.0, 1.645])
    roll = G.particle_rollout(gm, x0, U, particles=P, seed=SEED, call_index=CALL)
    stored = G.particle_cost(roll["particles"].permute(2, 0, 1, 3).contiguous(), U, cost, constraints=sc)
    assert bool(torch.isfinite(stored["cost"]).all()) and bool(torch.isfinite(stored["g"]).all())
    runs = [G.particle_evaluate(gm, x0, U, cost, constraints=sc, particles=P, seed=SEED, call_index=CALL, chunk=c) for c in (64, 0, 0)]
    for r in runs:                                                       # chunk = 64, the default, and the default again
        for k in ("cost", "stage", "g"):
            assert torch.equal(r[k], stored[k]), (kind, P, k)
    for b in range(B):                                                    # a plan alone has the bits it has inside the batch
        one = G.particle_evaluate(gm, x0[b], U[b], cost, constraints=sc, particles=P, seed=SEED, call_index=CALL)
        assert torch.equal(one["cost"][0], stored["cost"][b]) and torch.equal(one["stage"][0], stored["stage"][b]) and torch.equal(one["g"][0], stored["g"][b])
    other = G.particle_evaluate(gm, x0, U, cost, constraints=sc, particles=P, seed=SEED, call_index=CALL + 1)
    assert not torch.equal(other["cost"], stored["cost"])               # (the call index reaches the noise)
    free = G.particle_evaluate(gm, x0, U, cost, particles=P, seed=SEED, call_index=CALL)
    assert free["g"] is None and torch.equal(free["cost"], stored["cost"])


# ------------------------------------------------------------------------------------------------------------------ 4. the solve
def _solve_problem(G, b):
    import test_gpu_particles as TP
    m = TP.model_data(70, 2, 1, "pergp")
    kw = dict(gamma=0.7, Q=np.array([[1.0, 0.2], [0.2, 0.6]]), R=np.array([[0.3]]), x_ref=np.array([0.1, -0.1]), u_ref=np.array([0.05]))
    rows = (np.array([[1.0, 0.0], [0.3, -0.8]]), np.array(b), np.array([0.0, 1.645]))
    return m, TP.device_model(G, m), kw, rows


@pytest.mark.parametrize("b", [(0.45, 0.3), (0.95, 1.09)], ids=["restoration", "feasible"])
def test_solve_is_the_chain_of_its_parts_and_the_reference_search(G, b):
    """Two bounds: one no sample of the search meets (feasibility restoration throughout), and one that the reference's first batch meets
    with a few of its 16 samples (its margins there span 0.87 ... 1.02 and 1.03 ... 1.16), so that costs decide."""
    from gaussian_process_mpc_amd.mppi import mppi_sample, mppi_start, mppi_update
    m, gm, kw, rows = _solve_problem(G, b)
    K, P, Hh, iters = 16, 64, 4, 3
    x0 = np.array([0.3, -0.2])
    opt = dict(sigma=0.5, decay=0.8, beta=0.2, seed=5, call_index=3, lb=-1.0, ub=1.0)
    cost = G.CostParams(kw["gamma"], kw["Q"], kw["R"], x_ref=kw["x_ref"], u_ref=kw["u_ref"])
    sc = G.StateConstraints(rows[0], rows[1], kappa=rows[2])
    whole = G.mppi_solve_particles(gm, x0, np.zeros((Hh, 1)), cost, constraints=sc, particles=P, samples=K, iterations=iters, **opt)
    mean = torch.zeros((Hh, 1), dtype=torch.float64, device="cuda")
    best, trace = mppi_start(mean), []
    for it in range(iters):
        U = mppi_sample(mean, K, opt["sigma"], opt["lb"], opt["ub"], seed=opt["seed"], call_index=opt["call_index"], iteration=it, decay=opt["decay"])
        r = G.particle_evaluate(gm, x0, U, cost, constraints=sc, particles=P, seed=opt["seed"], call_index=opt["call_index"])
        up = mppi_update(U, r["cost"], best, opt["beta"], g=r["g"], mean=mean)
        mean, best = up["mean"], up["best"]
        trace.append(up["trace"].cpu().numpy())
    best, trace = best.cpu().numpy(), np.array(trace)
    print("  solve: key (%g, %.9f); parts: key (%g, %.9f); feasible per iteration %s" % (whole["violation"], whole["cost"], best[0], best[1], trace[:, 2]))
    assert np.array_equal(whole["trace"].view(np.int64), trace.view(np.int64)) and np.array_equal(whole["U"].reshape(-1).view(np.int64), best[2:].view(np.int64))
    assert (whole["violation"], whole["cost"]) == (best[0], best[1]) and np.all(np.isfinite(whole["trace"]))
    assert whole["feasible"] == (b[0] > 0.9) and (trace[:, 2] > 0).all() == (b[0] > 0.9)
    # the same search over the long double particle reference: the project's cost tolerance, 1e-6 relative (tests/test_gpu_mppi.py)
    ref = MR.solve(PC.evaluate(m, x0, Hh, P, opt["seed"], opt["call_index"], kw, cons=rows), np.zeros(Hh), K, 1, iters, opt["sigma"], opt["decay"],
                   opt["beta"], opt["seed"], opt["call_index"], opt["lb"], opt["ub"])
    print("  reference: key (%g, %.9f)" % (ref["violation"], ref["cost"]))
    assert np.array_equal(whole["trace"][:, 2:4], ref["trace"][:, 2:4])                        # feasible and alive samples per iteration
    np.testing.assert_allclose(whole["trace"][:, [0, 1, 4, 5]], ref["trace"][:, [0, 1, 4, 5]], rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(whole["U"].reshape(-1), ref["U"], rtol=0, atol=1e-9)
    assert abs(whole["cost"] - ref["cost"]) <= 1e-6 * abs(ref["cost"])


# ------------------------------------------------------------------------------------------------------------------ 5. the controller
def _mpc_c1(G, nominal=False):
    from gaussian_process_mpc_amd.synth import synth_problem
    ds, da, Hh = 2, (1 if nominal else 2), (4 if nominal else 10)
    pb = synth_problem(1, 100, ds, da, Hh, 64)
    mpc = G.RiskSensitiveMPC(0.5, Hh, ds, da, pb["Q"], pb["R"], nominal_models=G.LinearNominalModel.identity(ds, da) if nominal else None)
    for a, g in enumerate(mpc.dynamics.gpr_err):
        g.set_lambdas(pb["lambdas"][a])
        g.set_sigma_n(float(pb["sigma_n"][a]))
        g.set_sigma_f(1.0)
    mpc.dynamics.append_train_data(pb["X"][:, :ds], pb["X"][:, ds:], pb["Y"])
    mpc.set_lb([-1.0] * da)
    mpc.set_ub([1.0] * da)
    mpc.mppi_options = dict(mpc.mppi_options, samples=16, iterations=3, seed=4)
    mpc.particle_options = {"particles": 64}
    return mpc, pb


def test_controller_on_particles(G):
    mpc, pb = _mpc_c1(G)
    Hh, ds, da, x0 = 10, 2, 2, pb["x0"][0]
    mpc.set_state_constraints(np.array([[1.0, 0.0]]), [0.5], prob=0.95)
    mpc.propagation, mpc.solver = "particles", "mppi"
    U = mpc.get_optimal_trajectory(x0)
    assert U.shape == (Hh, da) and np.all(np.isfinite(U)) and np.all(np.abs(U) <= 1.0)
    assert mpc.solver_used == "mppi-particles x16 P64" and mpc.last_solve_info["trace"].shape == (3, 6)
    # evaluate_batch is particle_evaluate under (mppi_options seed, solve count)
    Ub = np.stack([U, 0.5 * U, np.zeros_like(U)])
    r = mpc.evaluate_batch(Ub, x0, constraints=True)
    want = G.particle_evaluate(mpc.dynamics, x0, Ub, mpc._cost_params(), constraints=mpc.state_constraints, particles=64, seed=4, call_index=mpc._solve_count)
    assert r["grad"] is None and torch.equal(r["cost"], want["cost"]) and torch.equal(r["g"], want["g"]) and r["g"].shape == (3, Hh, 1)
    assert mpc.evaluate_batch(Ub, x0)["g"] is None
    assert mpc.objective(U.reshape(-1)) == float(want["cost"][0].item())
    assert np.array_equal(mpc.constraints(U.reshape(-1)), want["g"][0].cpu().numpy().reshape(-1))
    # validate_plan: the new keys are particle_cost on its particles, the old keys are those of a call under moment matching
    v = mpc.validate_plan(U=U, x0=x0, particles=300, seed=9)
    roll = G.particle_rollout(mpc.dynamics, x0, U, particles=300, seed=9)
    pc = G.particle_cost(roll["particles"].permute(2, 0, 1, 3).contiguous(), U[None], mpc._cost_params(), constraints=mpc.state_constraints)
    assert v["cost_mc"] == float(pc["cost"][0].item()) and np.array_equal(v["stage_mc"], pc["stage"][0].cpu().numpy()) and v["stage_mc"].shape == (Hh + 1,)
    assert np.array_equal(v["g_mc"], pc["g"][0].cpu().numpy()) and v["g_mc"].shape == (Hh, 1)
    mpc.propagation = "moment_matching"
    old = mpc.validate_plan(U=U, x0=x0, particles=300, seed=9)
    for k in ("mean_mm", "var_mm", "mean_mc", "var_mc", "z_mean", "z_var", "se_mean", "se_var", "clamped", "stage_cost", "satisfaction", "requested",
              "joint_satisfaction", "particles"):
        assert np.array_equal(np.asarray(old[k]), np.asarray(v[k])), k
    assert old["cost_mc"] == v["cost_mc"]
    mpc.clear_state_constraints()
    assert "g_mc" not in mpc.validate_plan(U=U, x0=x0, particles=64, seed=9)
    # refusals
    mpc.propagation = "particles"
    x = U.reshape(-1)
    for call in (lambda: mpc.gradient(x), lambda: mpc.jacobian(x), lambda: mpc.get_optimal_trajectory(x0, solver="lbfgs"),
                 lambda: mpc.get_optimal_trajectory(x0, solver="auglag")):
        with pytest.raises(NotImplementedError, match=r"particles.*solver='mppi'"):
            call()
    mpc.solver = None
    with pytest.raises(NotImplementedError, match=r"particles.*solver='mppi'"):
        mpc.get_optimal_trajectory(x0)
    mpc.solver = "mppi"
    mpc.full_covariance = True                                            # not consulted
    assert mpc.get_optimal_trajectory(x0).shape == (Hh, da)
    mpc.full_covariance = False
    mpc.set_feedback_gain(np.zeros((da, ds)))
    with pytest.raises(ValueError, match="feedback gain"):
        mpc.get_optimal_trajectory(x0)
    mpc.clear_feedback_gain()
    mpc.propagation = "bogus"
    with pytest.raises(ValueError, match="'particles'"):
        mpc.get_optimal_trajectory(x0)


def test_nominal_model_controller_solves_on_particles(G):
    mpc, pb = _mpc_c1(G, nominal=True)
    mpc.propagation, mpc.solver = "particles", "mppi"
    mpc.set_state_constraints(np.array([[1.0, 0.0]]), [2.0], prob=0.9)
    U = mpc.get_optimal_trajectory(pb["x0"][0])
    assert U.shape == (4, 1) and np.all(np.isfinite(U)) and mpc.solver_used == "mppi-particles x16 P64"
    assert np.isfinite(mpc.last_solve_info["cost"])
    mpc.propagation = "moment_matching_full"                              # the refusal of nominal packs there stays
    with pytest.raises(NotImplementedError, match="nominal"):
        mpc.get_optimal_trajectory(pb["x0"][0])
