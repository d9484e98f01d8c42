"""GPU tests of the commanded input under a linear state feedback -- the input cost tr(R K Sigma K^T), the input chance constraints and the
rollout entry that carries both -- against tests/feedback_inputs_reference.py (long double; include/gpmpc.h, "Linearised propagation, full
covariance: the commanded input"; kernels in csrc/linprop_inputs.hip).

Shapes: the models of cases a (ds 2, da 1; one gain), b (ds 3, da 2: a non-symmetric R, two gain rows; per-step gains) and d (nominal +
noise, a non-diagonal init_cov, a cost schedule) of tests/test_gpu_linprop.py at H = 3, the shortest horizon with a column that is
propagated through two steps, and cases a and b at H = 33 (33 and 66 columns: the second 64-column block of the sweep).  Three rows per
case: one with kappa = 0, one not axis-aligned.  Every rollout check runs under the TILE and under the STREAM form of stage A.

Bounds: those of tests/test_gpu_linprop_fc.py.  Every sum within 1e-12 sum |terms| of the long double reference evaluated on the arrays the
device returned, plus 4 ulp of the value; structural zeros and the direct part c_rj exact; what the header states bit for bit is held
bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import feedback_inputs_reference as I
import linprop_fc_reference as F
import linprop_reference as R
import test_gpu_linprop as TL
import test_gpu_linprop_fc as TF
import test_host_feedback_inputs as HI
import test_host_linprop_fc as HF

pytestmark = pytest.mark.gpu
TOL, ULP, f64 = 1e-12, 2.0 ** -52, R.G.to_f64
case_model, device_model, same_bits = TL.case_model, TL.device_model, TL.same_bits
FORMS = ["tile", "stream"]
SHAPES = [("a", 3, 3, False, False), ("b", 2, 3, True, False), ("d", 3, 3, True, True), ("a", 2, 33, False, False), ("b", 2, 33, True, False)]


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    return g


def rows(G, da, rng):
    """Three rows: an upper bound on the first input, a mean-only (kappa = 0) lower bound on the last, one that is not axis-aligned."""
    C = np.concatenate([np.eye(da)[:1], -np.eye(da)[-1:], rng.uniform(0.3, 1.0, (1, da)) * np.where(np.arange(da) % 2, -1.0, 1.0)])
    return G.InputConstraints(C, [1.5, 1.2, 0.8], kappa=[1.6, 0.0, 2.0])


def within(got, want, unit):
    """Worst |got - want| / (1e-12 unit + 4 ulp |want|); where the unit is zero the entries are equal."""
    got, want, unit = np.asarray(got), f64(want), f64(unit)
    b = TOL * unit + 4 * ULP * np.abs(want)
    assert np.array_equal(got[b == 0], want[b == 0])
    return float((np.abs(got - want)[b > 0] / b[b > 0]).max()) if np.any(b > 0) else 0.0


def raw_rollout_inputs(G, gm, x0, U, K, cp, sc, grad, form):
    """gpmpc_linearised_fc_rollout_inputs with nothing asked (input_cost = 0, ucons_host = NULL), through ctypes."""
    from gaussian_process_mpc_amd import _lib
    from gaussian_process_mpc_amd.linearised import _gain, linearised_form, packed_dim
    from gaussian_process_mpc_amd.particles import _dev, _empty, _vp, _workspace
    dev = gm.device
    ds, da = gm.ds, gm.da
    U, x0 = _dev(U, dev), _dev(x0, dev)
    B, H = U.shape[0], U.shape[1]
    Kd, ks = _gain(K, H, ds, da, dev)
    p = packed_dim(ds)
    out = {"means": _empty(dev, B, H + 1, ds), "covs": _empty(dev, B, H + 1, ds, ds), "cost": _empty(dev, B), "g": _empty(dev, B, H, sc.m)}
    if grad:
        out.update(jac=_empty(dev, B, H, p, p + da), grad=_empty(dev, B, H, da), g_jac=_empty(dev, B, H * sc.m, H * da))
    flags = _lib.WANT_GRAD if grad else 0
    L = _lib.lib()
    with torch.cuda.device(dev), linearised_form(form):
        nb = L.gpmpc_linearised_fc_rollout_inputs_workspace_bytes(ctypes.byref(gm.c), B, H, flags, 0, 0, None)
        assert nb == L.gpmpc_linearised_fc_rollout_workspace_bytes(ctypes.byref(gm.c), B, H, flags, 0)
        ws = _workspace(dev, nb)
        _lib.check(L.gpmpc_linearised_fc_rollout_inputs(
            ctypes.byref(gm.c), B, H, _lib.ptr(x0), _vp(U), _vp(Kd), ks, ctypes.byref(cp.c), ctypes.byref(sc.c), flags, _vp(out["means"]),
            _vp(out["covs"]), _vp(out.get("jac")), _vp(out["cost"]), _vp(out.get("grad")), _vp(out["g"]), _vp(out.get("g_jac")), 0, None, None, None,
            0, _vp(ws), nb, _lib.stream_ptr(dev)), "gpmpc_linearised_fc_rollout_inputs")
    return out


# ------------------------------------------------------------------------------------------------------------------ the rollout
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,B,H,per_step,schedule", SHAPES)
def test_rollout_inputs_against_reference_and_bit_for_bit(G, name, B, H, per_step, schedule, form):
    from gaussian_process_mpc_amd._lib import lib, ptr, stream_ptr, check
    m = TF.roll_model(name)
    gm = device_model(G, m)
    ds, da, _ = R.dims(m)
    rng = np.random.default_rng(23)
    x0, U = rng.uniform(-1.0, 1.0, (B, ds)), rng.uniform(-1.0, 1.0, (B, H, da))
    if H > 3:
        U *= 0.3                                                             # (a long horizon stays in the data's range)
    K = rng.uniform(-0.5, 0.5, (H, da, ds) if per_step else (da, ds))
    cp, (gamma, Q, Rm), kw = TL.cost_case(G, m, H, rng, schedule)
    sc = G.StateConstraints(rng.standard_normal((2, ds)), rng.uniform(0.0, 0.5, 2), kappa=[1.5, 0.0])
    ic = rows(G, da, rng)
    base = dict(want_jac=True, constraints=sc, feedback=K, form=form)
    r = G.linearised_rollout(gm, x0, U, cp, input_cost=True, input_constraints=ic, **base)
    old = G.linearised_rollout(gm, x0, U, cp, **base)                        # gpmpc_linearised_fc_rollout, untouched
    assert r["g_u"].shape == (B, H, 3) and r["g_u_jac"].shape == (B, 3 * H, H * da) and "g_u" not in old
    # the old entry == the new entry with nothing asked; the trajectory and the state rows never see the inputs
    raw = raw_rollout_inputs(G, gm, x0, U, K, cp, sc, True, form)
    for k in ("means", "covs", "jac", "cost", "grad", "g", "g_jac"):
        assert same_bits(raw[k], old[k]), k
    for k in ("means", "covs", "jac", "g", "g_jac"):
        assert same_bits(r[k], old[k]), k
    # chunk = 64, two calls, one option at a time
    r64 = G.linearised_rollout(gm, x0, U, cp, input_cost=True, input_constraints=ic, chunk=64, **base)
    r2 = G.linearised_rollout(gm, x0, U, cp, input_cost=True, input_constraints=ic, **base)
    for k in r:
        assert same_bits(r[k], r64[k]) and same_bits(r[k], r2[k]), k
    rc_only = G.linearised_rollout(gm, x0, U, cp, input_cost=True, **base)
    ru_only = G.linearised_rollout(gm, x0, U, cp, input_constraints=ic, **base)
    assert same_bits(rc_only["cost"], r["cost"]) and same_bits(rc_only["grad"], r["grad"]) and "g_u" not in rc_only
    assert same_bits(ru_only["cost"], old["cost"]) and same_bits(ru_only["grad"], old["grad"])
    assert same_bits(ru_only["g_u"], r["g_u"]) and same_bits(ru_only["g_u_jac"], r["g_u_jac"])
    # objective only: the same bits, no Jacobians
    ro = G.linearised_rollout(gm, x0, U, cp, want_grad=False, constraints=sc, feedback=K, form=form, input_cost=True, input_constraints=ic)
    assert same_bits(ro["cost"], r["cost"]) and same_bits(ro["g_u"], r["g_u"]) and same_bits(ro["g"], r["g"]) and same_bits(ro["covs"], r["covs"])
    assert "grad" not in ro and "g_u_jac" not in ro
    rawo = raw_rollout_inputs(G, gm, x0, U, K, cp, sc, False, form)
    oldo = G.linearised_rollout(gm, x0, U, cp, want_grad=False, constraints=sc, feedback=K, form=form)
    for k in ("means", "covs", "cost", "g"):
        assert same_bits(rawo[k], oldo[k]), k
    # the pure functions on the returned arrays, bit for bit
    Ud = torch.as_tensor(U, device="cuda")
    pc = G.feedback_input_cost(cp, r["covs"], K, da)
    assert same_bits(r["cost"], old["cost"] + pc["c"]), "out_cost is not cost_plain + c, one rounding"
    assert same_bits(G.feedback_input_cost(cp, r["covs"], K, da, want_dcovs=False)["c"], pc["c"])
    cost = torch.empty(B, dtype=torch.float64, device="cuda")
    dm, dc, du = torch.empty_like(r["means"]), torch.empty_like(r["covs"]), torch.empty_like(Ud)
    check(lib().gpmpc_cost_grad(B, H, ds, da, ctypes.byref(cp.c), ptr(r["means"]), ptr(r["covs"]), ptr(Ud), ptr(cost), ptr(dm), ptr(dc), ptr(du),
                                stream_ptr()), "gpmpc_cost_grad")
    assert same_bits(r["grad"], du + G.linearised_fc_vjp(r["jac"], dm, dc + pc["dcovs"], ds, da)), "out_grad is not d_U + vjp(d_covs + out_dcovs)"
    pu = G.feedback_input_constraints(Ud, r["covs"], r["jac"], ic, K)
    assert same_bits(pu["g_u"], r["g_u"]) and same_bits(pu["g_u_jac"], r["g_u_jac"])
    assert same_bits(G.feedback_input_constraints(Ud, r["covs"], None, ic, K)["g_u"], r["g_u"])
    # against the long double reference on the returned arrays
    means, covs, jacs = r["means"].cpu().numpy(), r["covs"].cpu().numpy(), r["jac"].cpu().numpy()
    rc, ru = I.input_cost(covs, K, Rm), I.input_constraints(U, covs, jacs, K, ic.C, ic.d, ic.kappa)
    w = {"c": within(pc["c"].cpu().numpy(), rc["c"], rc["A_c"]), "seed": within(pc["dcovs"].cpu().numpy(), rc["dcovs"], rc["A_dcovs"]),
         "g_u": within(r["g_u"].cpu().numpy(), ru["g"], ru["A_g"]), "g_u_jac": within(r["g_u_jac"].cpu().numpy(), ru["gjac"], ru["A_gjac"])}
    assert not np.any(pc["dcovs"][:, H].cpu().numpy())
    ref = F.adjoint(jacs, means, covs, U, gamma, Q, Rm, **kw)
    gU = F.sweep(jacs, ref["dmu"], ref["dsig"] + rc["dcovs"])[0]
    aU = F.sweep(np.abs(jacs), None, rc["A_dcovs"])[0]
    tot = C_total = f64(ref["cost"] + rc["c"])
    w["cost"] = float((np.abs(r["cost"].cpu().numpy() - tot) / (TOL * f64(ref["A_cost"] + rc["A_c"]) + 4 * ULP * np.abs(C_total))).max())
    dU = ref["grad"] - F.sweep(jacs, ref["dmu"], ref["dsig"])[0]              # the direct part of the reference gradient
    w["grad"] = float((np.abs(r["grad"].cpu().numpy() - f64(dU + gU)) / (TOL * f64(ref["A_grad"] + aU))).max())
    print("  case %s H %d%s [%s]: of the bound: %s" % (name, H, " + schedule" if schedule else "", form,
                                                        ", ".join("%s %.3g" % kv for kv in w.items())))
    assert max(w.values()) <= 1.0
    # causality: blocks tau > t are exact zeros, sign included; tau = t is c_rj; row t = 0 has only its tau = 0 block
    gj = r["g_u_jac"].cpu().numpy().reshape(B, H, 3, H, da)
    for t in range(H):
        assert not np.any(gj[:, t, :, t + 1:]) and not np.any(np.signbit(gj[:, t, :, t + 1:])), t
        assert np.array_equal(gj[:, t, :, t], np.broadcast_to(ic.C, (B, 3, da))), t
    assert np.any(gj[:, 2, 0, 0] != 0.0) and np.any(gj[:, 2, 2, 0] != 0.0) and not np.any(gj[:, :, 1, :][:, np.tril_indices(H, -1)[0], np.tril_indices(H, -1)[1]])
    # a deliberate mistake of the reference is seen by the same bounds
    bad = I.input_constraints(U, covs, jacs, K, ic.C, ic.d, ic.kappa, offdiag_once=True)
    b = TOL * f64(ru["A_gjac"]) + 4 * ULP * np.abs(f64(ru["gjac"]))
    miss = float((np.abs(r["g_u_jac"].cpu().numpy() - f64(bad["gjac"]))[b > 0] / b[b > 0]).max())
    print("  case %s H %d [%s]: the reference with offdiag_once misses by %.3g bounds" % (name, H, form, miss))
    assert miss >= 100.0


@pytest.mark.parametrize("form", FORMS)
def test_nan_plan_poisons_its_own_later_steps_only(G, form):
    m = TF.roll_model("a")
    gm = device_model(G, m)
    rng = np.random.default_rng(3)
    x0, U, K = rng.uniform(-1, 1, (3, 2)), rng.uniform(-1, 1, (3, 3, 1)), rng.uniform(-0.5, 0.5, (1, 2))
    ic = rows(G, 1, rng)
    good = G.linearised_rollout(gm, x0, U, None, feedback=K, input_constraints=ic, form=form)
    Un = U.copy()
    Un[1, 1, 0] = np.nan
    bad = G.linearised_rollout(gm, x0, Un, None, feedback=K, input_constraints=ic, form=form)
    g = bad["g_u"].cpu().numpy()
    assert np.all(np.isnan(g[1, 1:])) and np.all(np.isfinite(g[1, 0])) and same_bits(bad["g_u"][1, 0], good["g_u"][1, 0])
    for b in (0, 2):
        assert same_bits(bad["g_u"][b], good["g_u"][b]) and same_bits(bad["g_u_jac"][b], good["g_u_jac"][b]), b
    gj = bad["g_u_jac"][1].cpu().numpy().reshape(3, 3, 3)
    assert np.array_equal(gj[0], good["g_u_jac"][1].cpu().numpy().reshape(3, 3, 3)[0])


def test_zero_gain_row_and_no_gain(G):
    """A gain whose second row is zero: a row on that input alone has sd = 0 exactly and a Jacobian that is the direct part only.  No gain at
    all: every row is c . v - d."""
    m = TF.roll_model("b")
    gm = device_model(G, m)
    rng = np.random.default_rng(8)
    B, H = 2, 3
    x0, U = rng.uniform(-1, 1, (B, 3)), rng.uniform(-1, 1, (B, H, 2))
    K = rng.uniform(-0.5, 0.5, (2, 3))
    K[1] = 0.0
    ic = G.InputConstraints([[0.0, 1.0], [1.0, 0.0]], [0.7, 0.7], kappa=2.0)
    r = G.linearised_rollout(gm, x0, U, None, feedback=K, input_constraints=ic)
    g, gj = r["g_u"].cpu().numpy(), r["g_u_jac"].cpu().numpy().reshape(B, H, 2, H, 2)
    assert np.array_equal(g[:, :, 0], U[:, :, 1] - 0.7)
    assert np.all(g[:, 1:, 1] > U[:, 1:, 0] - 0.7)                           # (Sigma_0 = init_cov may be zero: from step 1 on)
    direct = np.zeros((B, H, H, 2))
    for t in range(H):
        direct[:, t, t, 1] = 1.0
    assert np.array_equal(gj[:, :, 0], direct) and np.any(gj[:, 2, 1, 0] != 0.0)
    r0 = G.linearised_rollout(gm, x0, U, None, input_constraints=ic)
    assert np.array_equal(r0["g_u"].cpu().numpy(), np.stack([U[:, :, 1] - 0.7, U[:, :, 0] - 0.7], axis=-1))
    cp = G.CostParams(0.5, np.eye(3), np.eye(2))
    assert not np.any(G.feedback_input_cost(cp, r0["covs"], None, 2)["c"].cpu().numpy())
    assert same_bits(G.linearised_rollout(gm, x0, U, cp, input_cost=True)["cost"], G.linearised_rollout(gm, x0, U, cp, full_covariance=True)["cost"])


def test_feedback_tightens_the_input_bounds_and_costs(G):
    """The unstable plant of test_lqr_gain_and_feedback_shrink_the_prediction: a nominal plan strictly inside the box has c . v - d < 0 on
    every row and g_u > 0 on at least one, and input_cost raises the cost by the reference's c."""
    m = HF.unstable_model()
    gm = device_model(G, m)
    K = G.lqr_gain(gm, np.zeros(2), np.zeros(1), np.eye(2), np.eye(1))
    x0, U = np.array([[0.1, -0.1]]), np.full((1, 6, 1), 0.9)
    ic = G.InputConstraints.box([-1.0], [1.0], 1, prob=0.95)
    cp = G.CostParams(0.5, np.eye(2), [[0.7]])
    r = G.linearised_rollout(gm, x0, U, cp, feedback=K, input_cost=True, input_constraints=ic, want_grad=False)
    plain = G.linearised_rollout(gm, x0, U, cp, feedback=K, want_grad=False)
    nominal = np.einsum("rj,btj->btr", ic.C, U) - ic.d
    g = r["g_u"].cpu().numpy()
    print("  nominal margins %s, g_u of the upper bound %s" % (nominal[0, :, 0], g[0, :, 0]))
    assert np.all(nominal < 0) and np.any(g > 0) and np.all(g > nominal)
    rc = I.input_cost(r["covs"].cpu().numpy(), K, [[0.7]])
    c_dev = G.feedback_input_cost(cp, r["covs"], K, 1, want_dcovs=False)["c"]
    assert same_bits(r["cost"], plain["cost"] + c_dev) and within(c_dev.cpu().numpy(), rc["c"], rc["A_c"]) <= 1.0
    assert float(c_dev.item()) > 0 and r["cost"].item() > plain["cost"].item()


# ------------------------------------------------------------------------------------------------------------------ MPC
def test_mpc_stacks_the_blocks_and_refuses_other_propagations(G):
    mpc, pb = TL._mpc(G)
    H = mpc.horizon
    U = np.ascontiguousarray(pb["U"][:, :H])
    x = U[0].reshape(-1)
    mpc.propagation = "linearised_full"
    K = G.lqr_gain(mpc.dynamics, pb["x0"][0], U[0, 0], np.eye(2), np.eye(1))
    mpc.set_feedback_gain(K)
    c_plain = mpc.objective(x)
    assert mpc.constraints(x) == 0
    mpc.set_input_chance_bounds(0.95)                                        # lb = -2, ub = 2: two rows
    ic = mpc.input_constraints
    assert ic.m == 2 and np.array_equal(ic.C, [[1.0], [-1.0]]) and np.array_equal(ic.d, [2.0, 2.0])
    kw = dict(feedback=K, input_constraints=ic)
    r1 = G.linearised_rollout(mpc.dynamics, mpc.curr_state, U[:1], mpc._cost_params(), **kw)
    assert mpc.objective(x) == c_plain == r1["cost"][0].item()
    assert np.array_equal(np.asarray(mpc.constraints(x)), r1["g_u"][0].cpu().numpy().reshape(-1))          # the input block alone
    assert np.array_equal(np.asarray(mpc.jacobian(x)), r1["g_u_jac"][0].cpu().numpy().reshape(-1))
    mpc.set_state_constraints(np.array([[1.0, 0.0]]), [0.4], prob=0.9)
    mpc.feedback_input_cost = True
    r1 = G.linearised_rollout(mpc.dynamics, mpc.curr_state, U[:1], mpc._cost_params(), constraints=mpc.state_constraints, input_cost=True, **kw)
    c = mpc.objective(x)
    assert c == r1["cost"][0].item() and c > c_plain and np.array_equal(np.asarray(mpc.gradient(x)), r1["grad"][0].cpu().numpy())
    g, J = np.asarray(mpc.constraints(x)), np.asarray(mpc.jacobian(x))
    assert g.shape == (H * 3,) and J.shape == (H * 3 * H,)
    assert np.array_equal(g, np.concatenate([r1["g"][0].cpu().numpy().reshape(-1), r1["g_u"][0].cpu().numpy().reshape(-1)]))
    eb = mpc.evaluate_batch(U, constraints=True)
    assert np.array_equal(J.reshape(3 * H, H), np.concatenate([eb["g_jac"][0].cpu().numpy(), eb["g_u_jac"][0].cpu().numpy()], axis=0))
    assert same_bits(eb["g_u"][:1], r1["g_u"]) and same_bits(eb["cost"][:1], r1["cost"])
    nb = mpc.evaluate_batch(U)
    assert "g_u" not in nb and same_bits(nb["cost"], eb["cost"])
    mpc.set_input_constraints([[1.0]], [1.5], kappa=1.0)
    assert mpc.input_constraints.m == 1 and np.asarray(mpc.constraints(x)).shape == (H * 2,)
    mpc.set_input_chance_bounds(0.95)
    # the solvers that take it
    mpc.mppi_options.update(samples=16, iterations=2)
    plan = mpc.get_optimal_trajectory(pb["x0"][0], solver="mppi")
    assert plan.shape == (H, 1) and np.all(np.isfinite(plan)) and np.isfinite(mpc.last_solve_info["cost"])
    with pytest.raises(NotImplementedError, match="multi-start"):
        mpc.get_optimal_trajectory(pb["x0"][0], n_starts=2)
    # the refusals under other propagations
    for prop in ("linearised", "moment_matching", "moment_matching_full", "particles"):
        mpc.clear_feedback_gain()
        mpc.propagation = prop
        with pytest.raises(ValueError, match="linearised_full"):
            mpc.objective(x)
        mpc.feedback_input_cost = False
        with pytest.raises(ValueError, match="linearised_full"):
            mpc.evaluate_batch(U)
        mpc.clear_input_constraints()
        mpc.feedback_input_cost = True
        with pytest.raises(ValueError, match="linearised_full"):
            mpc.objective(x)
        mpc.set_input_chance_bounds(0.95)
    mpc.clear_input_constraints()
    mpc.feedback_input_cost = False
    mpc.propagation = "linearised"
    assert np.isfinite(mpc.objective(x))
    with pytest.raises(ValueError, match="inputs"):
        mpc.set_input_constraints([[1.0, 0.0]], [1.0], prob=0.9)


def test_mppi_host_loop_matches_its_parts_with_both_options(G):
    from gaussian_process_mpc_amd.mppi import mppi_sample, mppi_start, mppi_update
    m = case_model("a")
    gm = device_model(G, m)
    ds, da, H, Ks, iters = 2, 1, 4, 8, 2
    rng = np.random.default_rng(5)
    cp, _, _ = TL.cost_case(G, m, H, rng)
    sc = G.StateConstraints(np.array([[1.0, 0.0]]), [0.3], kappa=1.0)
    ic = G.InputConstraints.box([-1.0], [1.0], 1, prob=0.9)
    x0, U0, K = rng.uniform(-0.5, 0.5, ds), rng.uniform(-0.5, 0.5, (H, da)), rng.uniform(-0.5, 0.5, (da, ds))
    kw = dict(sigma=0.4, lb=-1.0, ub=1.0, seed=17, call_index=3)
    s = G.mppi_solve_linearised(gm, x0, U0, cp, constraints=sc, samples=Ks, iterations=iters, decay=0.8, beta=0.2, feedback=K, input_cost=True,
                                input_constraints=ic, **kw)
    plain = G.mppi_solve_linearised(gm, x0, U0, cp, constraints=sc, samples=Ks, iterations=iters, decay=0.8, beta=0.2, feedback=K, **kw)
    mean = torch.as_tensor(U0, device="cuda")
    best = mppi_start(mean)
    for it in range(iters):
        U, x0b = mppi_sample(mean, Ks, iteration=it, decay=0.8, x0=x0, **kw)
        r = G.linearised_rollout(gm, x0b, U, cp, want_grad=False, want_traj=False, constraints=sc, feedback=K, input_cost=True, input_constraints=ic)
        u = mppi_update(U, r["cost"], best, 0.2, g=torch.cat([r["g"], r["g_u"]], -1), mean=mean)
        mean, best = u["mean"], u["best"]
    b = best.cpu().numpy()
    assert np.array_equal(s["U"].reshape(-1), b[2:]) and s["violation"] == b[0] and s["cost"] == b[1] and np.isfinite(s["cost"])
    assert s["cost"] != plain["cost"]
    big = G.InputConstraints(np.ones((16, 1)), np.ones(16), kappa=1.0)
    with pytest.raises(ValueError, match="exceed"):
        G.mppi_solve_linearised(gm, x0, U0, cp, constraints=sc, samples=Ks, iterations=1, feedback=K, input_constraints=big, **kw)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_c_refusals_on_the_device(G):
    """Every refusal of the header, with a device present: GPMPC_E_ARG before a launch (the pointers handed over are not device memory)."""
    from gaussian_process_mpc_amd import _lib
    n = HI.check_refusals(_lib.lib())
    torch.cuda.synchronize()                                             # nothing was enqueued: no fault surfaces here
    assert n >= 60


def test_python_refusals(G):
    m = case_model("a")
    gm = device_model(G, m)
    mu, cov, U, K = F.make_inputs(m, 3)
    with pytest.raises(TypeError, match="InputConstraints"):
        G.linearised_rollout(gm, mu, U[:, None, :], None, input_constraints=G.StateConstraints([[1.0]], [1.0], kappa=1.0))
    with pytest.raises(ValueError, match="inputs"):
        G.linearised_rollout(gm, mu, U[:, None, :], None, input_constraints=G.InputConstraints([[1.0, 1.0]], [1.0], kappa=1.0))
    with pytest.raises(ValueError, match="input_cost needs a cost"):
        G.linearised_rollout(gm, mu, U[:, None, :], None, input_cost=True)


# ------------------------------------------------------------------------------------------------------------------ particles under feedback
def particle_problem(G, P):
    m = TF.roll_model("b")                                                   # ds 3, da 2
    gm = device_model(G, m)
    rng = np.random.default_rng(31)
    B, H = 2, 3
    x0, U = rng.uniform(-1.0, 1.0, (B, 3)), rng.uniform(-1.0, 1.0, (B, H, 2))
    K = rng.uniform(-0.5, 0.5, (H, 2, 3))
    mu = G.linearised_rollout(gm, x0, U, None, want_grad=False, feedback=K)["means"]
    return m, gm, B, H, x0, U, K, mu


@pytest.mark.parametrize("P", [64, 300])
def test_particles_under_feedback(G, P):
    """The chain property, K = NULL == gpmpc_particle_rollout, the inputs against the long double v + K (x - mu), violation counts recomputed
    from the returned inputs (bounds placed in a gap, as tests/test_gpu_particles.py does for states), input_cov == K cov K^T."""
    m, gm, B, H, x0, U, K, mu = particle_problem(G, P)
    ds, da, seed, ci = 3, 2, 77, 2
    r = G.particle_rollout(gm, x0, U, particles=P, seed=seed, call_index=ci, feedback=K, mean_ref=mu)
    r2 = G.particle_rollout(gm, x0, U, particles=P, seed=seed, call_index=ci, feedback=K, mean_ref=mu, chunk=64)
    for k in ("particles", "inputs", "mean", "cov", "input_mean", "input_cov"):
        assert same_bits(r[k], r2[k]), k
    assert r["inputs"].shape == (B, P, H, da) and r["input_mean"].shape == (B, H, da) and r["input_cov"].shape == (B, H, da, da)
    # the chain: noise -> inputs -> step with inputs, bit for bit
    X = r["particles"]
    plain = G.particle_rollout(gm, x0, U, particles=P, seed=seed, call_index=ci)
    assert same_bits(X[:, :, 0], plain["particles"][:, :, 0]) and not same_bits(X[:, :, 2], plain["particles"][:, :, 2])
    x = X[:, :, 0].contiguous()
    Ud = torch.as_tensor(U, device="cuda")
    worst = 0.0
    for t in range(H):
        u = G.particle_inputs(x, Ud[:, t], torch.as_tensor(K[t], device="cuda"), mu[:, t])
        assert same_bits(u, r["inputs"][:, :, t]), t
        ref_u, A_u = I.particle_inputs(x.cpu().numpy(), U[:, t], K[t], mu[:, t].cpu().numpy())
        worst = max(worst, within(u.cpu().numpy(), ref_u, A_u))
        eps = G.particle_noise(P, da + ds, t + 1, seed=seed, call_index=ci)
        x = G.particle_step_inputs(gm, x, u, eps)[0]
        assert same_bits(x, X[:, :, t + 1]), t
    print("  P = %d: inputs against v + K (x - mu) in long double: %.3g of the bound" % (P, worst))
    assert worst <= 1.0
    # K = NULL: the particles of gpmpc_particle_rollout, and every particle's input is the plan's
    ic0 = rows(G, da, np.random.default_rng(1))
    r0 = G.particle_rollout(gm, x0, U, particles=P, seed=seed, call_index=ci, input_constraints=ic0)
    for k in ("particles", "mean", "cov"):
        assert same_bits(r0[k], plain[k]), k
    assert torch.equal(r0["clamped"], plain["clamped"])
    assert np.array_equal(r0["inputs"].cpu().numpy(), np.broadcast_to(U[:, None], (B, P, H, da)))
    assert same_bits(G.particle_inputs(x, Ud[:, 0]), Ud[:, 0][:, None].expand(B, P, da).contiguous())
    # (P equal values: their folded sum / P is the value to a few ulp, the deviations from it are of that size)
    assert np.abs(r0["input_mean"].cpu().numpy() - U).max() <= 8 * ULP * np.abs(U).max()
    assert np.abs(r0["input_cov"].cpu().numpy()).max() <= (8 * ULP * np.abs(U).max()) ** 2 * P / (P - 1)
    nom = np.einsum("rj,btj->btr", ic0.C, U) > ic0.d
    assert np.array_equal(r0["input_violation"].cpu().numpy(), nom.astype(np.float64))
    assert np.array_equal(r0["joint_input_violation"].cpu().numpy(), nom.any(axis=(1, 2)).astype(np.float64))
    # violation counts: rows whose bound sits in the widest gap around the 80 % quantile of c . u
    inp = r["inputs"].cpu().numpy()                                          # (B, P, H, da)
    C = np.array([[1.0, 0.0], [0.6, -0.8]])
    cu = np.einsum("rj,bptj->bptr", C.astype(np.longdouble), inp.astype(np.longdouble))
    d = np.empty(2)
    for r_ in range(2):
        v = np.sort(f64(cu[..., r_]).reshape(-1))
        k = int(0.8 * v.size)
        k = k - 3 + int(np.argmax(np.diff(v[k - 3:k + 4])))
        d[r_] = 0.5 * (v[k] + v[k + 1])
    g = f64(cu - d.astype(np.longdouble))
    assert np.abs(g).min() >= 1e-9, "an input sits on a constraint boundary: no case may be left out"
    ic = G.InputConstraints(C, d, kappa=0.0)
    rv = G.particle_rollout(gm, x0, U, particles=P, seed=seed, call_index=ci, feedback=K, mean_ref=mu, input_constraints=ic)
    assert same_bits(rv["inputs"], r["inputs"]) and same_bits(rv["particles"], r["particles"])
    viol = (g > 0).sum(axis=1) / P                                           # (B, H, rows)
    joint = (g > 0).any(axis=(2, 3)).sum(axis=1) / P
    assert np.array_equal(rv["input_violation"].cpu().numpy(), viol) and np.array_equal(rv["joint_input_violation"].cpu().numpy(), joint)
    assert np.any((viol > 0.0) & (viol < 1.0)) and np.any((joint > 0.0) & (joint < 1.0))
    # the stand-alone statistics on the same inputs: the same bits; exactly symmetric; mean and covariance against long double
    st = G.particle_input_stats(rv["inputs"].permute(2, 0, 1, 3).contiguous(), ic)
    for k in ("input_mean", "input_cov", "input_violation", "joint_input_violation"):
        assert same_bits(st[k], rv[k]), k
    ucov = rv["input_cov"]
    assert torch.equal(ucov, ucov.transpose(-1, -2))
    il = inp.astype(np.longdouble)
    mean_ref = il.mean(axis=1)
    dl = il - mean_ref[:, None]
    cov_ref = np.einsum("bpti,bptj->btij", dl, dl) / (P - 1)
    cov_abs = np.einsum("bpti,bptj->btij", np.abs(dl), np.abs(dl)) / (P - 1)
    assert within(rv["input_mean"].cpu().numpy(), mean_ref, np.abs(il).mean(axis=1)) <= 1.0
    # (each float64 difference u - mean rounds at the size of u, not of the difference: ulp (|u| + |mean|) |d| per factor, in units of tol)
    mag = np.abs(il) + np.abs(mean_ref)[:, None]
    sub = (ULP / TOL) * (np.einsum("bpti,bptj->btij", mag, np.abs(dl)) + np.einsum("bpti,bptj->btij", np.abs(dl), mag)) / (P - 1)
    assert within(ucov.cpu().numpy(), cov_ref, cov_abs + sub) <= 1.0
    # input_cov == K cov K^T of the returned particle covariance: an algebraic identity of the two sample covariances
    cov = r["cov"].cpu().numpy().astype(np.longdouble)[:, :H]
    Kl = K.astype(np.longdouble)
    want = np.einsum("tik,btkl,tjl->btij", Kl, cov, Kl)
    Xl = X.cpu().numpy().astype(np.longdouble)[:, :, :H]
    dx = np.abs(Xl - Xl.mean(axis=1)[:, None])
    unit = np.einsum("tik,bptk,bptl,tjl->btij", np.abs(Kl), dx, dx, np.abs(Kl)) / (P - 1)
    e = np.abs(f64(ucov.cpu().numpy() - want)) / (2 * (TOL * f64(unit) + 4 * ULP * np.abs(f64(want))))
    print("  P = %d: input_cov vs K cov K^T: %.3g of the bound between two float64 routes" % (P, e.max()))
    assert e.max() <= 1.0


def test_validate_plan_under_feedback(G):
    mpc, pb = TL._mpc(G)
    H = mpc.horizon
    U = np.ascontiguousarray(pb["U"][0, :H])
    base = mpc.validate_plan(U, pb["x0"][0], particles=512, seed=3)
    mpc.propagation = "linearised_full"
    with pytest.raises(ValueError, match="feedback gain"):
        mpc.validate_plan(U, pb["x0"][0], particles=512, seed=3, feedback=True)
    K = G.lqr_gain(mpc.dynamics, pb["x0"][0], U[0], np.eye(2), np.eye(1))
    mpc.set_feedback_gain(K)
    mpc.set_input_chance_bounds(0.95)
    same = mpc.validate_plan(U, pb["x0"][0], particles=512, seed=3)          # without feedback=True nothing changes
    assert set(same) == set(base) and all(np.array_equal(np.asarray(same[k]), np.asarray(base[k])) for k in base)
    v = mpc.validate_plan(U, pb["x0"][0], particles=512, seed=3, feedback=True)
    shapes = {"mean_lf": (H + 1, 2), "cov_lf": (H + 1, 2, 2), "input_cov_lf": (H, 1, 1), "input_mean_mc": (H, 1), "input_cov_mc": (H, 1, 1),
              "input_satisfaction": (H, 2), "input_requested": (2,)}
    for k, shp in shapes.items():
        assert v[k].shape == shp and np.all(np.isfinite(v[k])), k
    assert abs(v["input_requested"][0] - 0.95) < 1e-12 and 0.0 <= v["joint_input_satisfaction"] <= v["input_satisfaction"].min() <= 1.0
    assert np.isfinite(v["stage_cost"]) and v["stage_cost"] != base["stage_cost"] and not np.array_equal(v["mean_mc"], base["mean_mc"])
    r = G.linearised_rollout(mpc.dynamics, pb["x0"][0], U[None], None, want_grad=False, feedback=K)
    assert np.array_equal(v["mean_lf"], r["means"][0].cpu().numpy())
    Kh = K.reshape(1, 2)
    assert np.allclose(v["input_cov_lf"][:, 0, 0], np.einsum("k,tkl,l->t", Kh[0], v["cov_lf"][:H], Kh[0]), rtol=1e-12, atol=0)
    ratio = v["input_cov_mc"][:, 0, 0] / v["input_cov_lf"][:, 0, 0]
    print("  input variance, particles / linearised_full, steps 0...: %s" % ratio)
    assert np.all(np.isfinite(ratio)) and np.all(ratio > 0.0)
