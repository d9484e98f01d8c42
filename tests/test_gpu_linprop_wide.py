"""GPU tests of the model-based rollouts at D = state_dim + action_dim of 6, 7 and 8 (csrc/linprop.hip, linprop_stream.hip, linprop_fc.hip,
linprop_inputs.hip, the particle kernels), against the long double references tests/linprop_reference.py, linprop_fc_reference.py,
feedback_inputs_reference.py and particle_reference.py.  The neighbouring files stop at state_dim 3, action_dim 2, D = 5.

Cases: tests/linprop_wide_cases.py (w1 ... w7, each the smallest for what it names there).  What each reaches, read from the dispatch code
(these entries expose no plan): every case runs the runtime-D kernels of the diagonal step (k_lp_kstar, k_lp_quad, k_lp_sums, k_lp_hess,
k_lp_jac) under TILE and their k_lps_* counterparts under STREAM, then k_lpf_hess<D>, k_lpf_hfin, k_lpf_close and, in the rollouts,
k_lpf_vjp, k_lpf_constraints<DS, JAC>, k_rollout_constraints<DS, JAC> (the diagonal rule) and the cost kernels:
    w1  k_lpf_hess<8>; DS = 5; p = 20, nc = 23; five GpGroups of one; STREAM: a matrix per GP, 3 columns per group
    w2  k_lpf_hess<8>; DS = 7; p = 35, nc = 36 (k_lpf_vjp: 36 lanes, k_lpf_close: 1260 elements); one GpGroup of seven, ONE inverse:
        STREAM groups of four (column, GP) vectors, 35 vectors, the ninth group of three; n = 130: three row blocks, two 128-column chunks
    w3  k_lpf_hess<8>; DS = 6; three GpGroups {0,2,5} {1,4} {3}; the nominal weights in g; a non-diagonal init_cov; a cost schedule
    w4  k_lpf_hess<8> at action_dim = 0: U = NULL, p = nc = 44 (1936 elements a wave), NH = 36, no gain, no cost, no sweep
    w5  k_lpf_hess<8>; DS = 4; B = 65: two column tiles, and chunk = 64 leaves a second chunk of one column
    w6  k_lpf_hess<7>; DS = 2; H da = 65: two waves in k_rollout_constraints, k_lpf_constraints and k_lpi_constraints, tau = c / 5
    w7  k_lpf_hess<6>; DS = 3; a visibly non-symmetric inverse at three inputs
k_lpi_cost, k_lpi_constraints<DS, JAC>: w1, w3, w6.  k_pt_assemble, k_pt_finish at (3, 3) and (5, 3); k_lpi_pinputs at (5, 3).

Bounds: the project's, unchanged.  Every sum within 1e-12 sum |terms| of the long double reference, carried through the composite outputs
by the formulas of the references, plus 4 ulp of the sizes the last float64 additions round at; cost, gradient and constraints in the units
of tests/cost_reference.py, linprop_fc_reference.constraints and feedback_inputs_reference, as the neighbouring files apply them; a control
(a deliberate mistake of a reference) misses by at least 100 bounds.  tests/test_host_linprop_wide.py pins on the CPU that a float64
restatement of every reference passes these bounds at these cases (worst 3.9e-4 of a bound) and that every control fails them.

Worst ratios to the bound measured on an MI355X, per output class, over all cases (TILE | STREAM); the smallest control miss beside them:
    diagonal step        mean 1.4e-4 | 1.7e-4    var 8.8e-5 | 1.2e-4     Jacobian 2.4e-4 | 2.2e-4
                         controls: drop_h 9.5e9 (w1, w5), drop_nominal_g 1.3e13 (w3), r_twice 3.7e7 (w7)
    full step            mean 1.3e-4 | 1.3e-4    Sigma' 1.4e-4 | 1.4e-4  Jacobian 2.3e-4 | 2.3e-4
                         controls: drop_cross_hess 1.8e10 (w1), offdiag_once 5.6e10 (w2), feedback_cross_dropped 2.4e10 (w3), 7.7e9 (w6)
    diagonal rollout     cost 3.6e-5 | 7.3e-5    gradient 1.6e-4 | 1.5e-4    g 2.3e-4 | 2.1e-4    g_jac 3.1e-4 | 3.5e-4
                         against gpmpc_cost_grad + gpmpc_rollout_vjp (of twice the bound): cost 2.4e-5 | 2.5e-5, gradient 2.6e-5 | 2.6e-5
    full rollout         cost 4.9e-5 | 7.6e-5    gradient 8.5e-5 | 6.9e-5    g 2.3e-4 | 2.1e-4    g_jac 3.1e-4 | 3.5e-4
                         against gpmpc_cost_grad + gpmpc_linearised_fc_vjp: the same bits
    commanded input      c 6.2e-5 | 8.5e-5    seed 2.0e-4 | 2.0e-4    g_u 1.7e-4 | 1.7e-4    g_u_jac 8.3e-5 | 1.1e-4
                         cost 3.0e-5 | 4.8e-5    gradient 5.9e-5 | 6.9e-5
                         controls: offdiag_once 8.4e10 (w1, w3, w6), R_transposed 8.4e10 (w1), gain_of_next_step 3.4e12 (w6)
    particles            draw 1.8e-4, mean 2.0e-4, inputs 2.2e-4, draw and mean with an input per particle 1.3e-4, 1.5e-4
The worst of any case and class is 3.5e-4 of its bound (g_jac of w6 under STREAM); no kernel missed a bound, at any width."""
import functools

import numpy as np
import pytest
import torch

import feedback_inputs_reference as I
import linprop_fc_reference as F
import linprop_reference as R
import linprop_wide_cases as W
import particle_reference as PR
import test_gpu_feedback_inputs as TI
import test_gpu_linprop as TL
import test_gpu_linprop_fc as TF
import test_host_linprop_wide as HW

pytestmark = pytest.mark.gpu
TOL, ULP, f64 = 1e-12, 2.0 ** -52, R.G.to_f64
same_bits, device_model, within = TL.same_bits, TL.device_model, TI.within


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    return g


def cases(names=W.NAMES):
    return pytest.mark.parametrize("name", list(names))


forms = pytest.mark.parametrize("form", W.FORMS)


# ------------------------------------------------------------------------------------------------------------------ the steps
@forms
@cases()
def test_diagonal_step(G, name, form):
    """Values and Jacobian against R.step; chunk = 64, two calls and the call without the Jacobian bit for bit (``check_step``)."""
    from gaussian_process_mpc_amd.linearised import linearised_form
    m = W.model(name)
    gm = device_model(G, m)
    assert (gm.c.gp_stride == 0) == (name == "w2")
    B = W.WIDE[name]["B"]
    with linearised_form(form):
        ref = TL.check_step(G, gm, m, B, "%s [%s]" % (name, form), control=W.STEP_CONTROLS.get(name))
        w = TL.worst_step(ref, *(t.cpu().numpy() for t in G.linearised_step(gm, *R.make_inputs(m, B))))
        print("  %s [%s] diagonal step: mean %.3g, var %.3g, Jacobian %.3g of the bound" % ((name, form) + w))      # (the digits %.3f hides)
        if name == "w4":                                                     # action_dim = 0: no inputs at all is the same call
            mu, var, U = R.make_inputs(m, B)
            assert U.shape == (B, 0)
            assert all(same_bits(x, y) for x, y in zip(G.linearised_step(gm, mu, var, None), G.linearised_step(gm, mu, var, U)))


@forms
@cases()
def test_full_covariance_step(G, name, form):
    """Values and packed Jacobian against F.step with a gain (none at action_dim = 0); Sigma' exactly symmetric; out_mu carries the bits of
    the diagonal step; chunk = 64, two calls and the call without the Jacobian bit for bit (``check_step`` of test_gpu_linprop_fc.py)."""
    m = W.model(name)
    gm = device_model(G, m)
    B, gain = W.WIDE[name]["B"], W.WIDE[name]["da"] > 0
    ref = TF.check_step(G, gm, m, B, name, form, control=W.FULL_CONTROLS.get(name), gain=gain)
    w = TF.worst_step(ref, *(t.cpu().numpy() for t in G.linearised_step_full(gm, *F.make_inputs(m, B, gain=gain), form=form)))
    print("  %s [%s] full step: mean %.3g, Sigma' %.3g, Jacobian %.3g of the bound" % ((name, form) + w))


@cases(["w2", "w5"])
def test_stream_against_tile(G, name):
    """Both forms within the bounds of the one reference (they are not bit-equal by design), hence within twice the bound of each other."""
    m = W.model(name)
    gm = device_model(G, m)
    mu, var, U = R.make_inputs(m, W.WIDE[name]["B"])
    ref = R.step(m, mu, var, U)
    o = {f: [t.cpu().numpy() for t in G.linearised_step(gm, mu, var, U, form=f)] for f in W.FORMS}
    for f in o:
        w = TL.worst_step(ref, *o[f])
        print("  %s %s: mean %.3f, var %.3f, Jacobian %.3f of the bound" % ((name, f) + w))
        assert max(w) <= 1.0
    bounds = (TOL * f64(ref["m_abs"]), TOL * f64(ref["var_abs"]) + 4 * ULP * f64(ref["var_mag"]), TOL * f64(ref["jac_abs"]) + 4 * ULP * f64(ref["jac_mag"]))
    for k, b in enumerate(bounds):
        d = np.abs(o["tile"][k] - o["stream"][k])
        print("  %s tile vs stream, output %d: worst %.3f of twice the bound" % (name, k, float((d / np.where(b == 0, 1.0, 2 * b)).max())))
        assert np.all(d <= 2.0 * b)
    assert not all(np.array_equal(o["tile"][k], o["stream"][k]) for k in range(3))       # (the two forms were run: they do differ in bits)


@forms
@cases(["w1", "w2"])
def test_columns_are_independent(G, name, form):
    """Column c of the batch has the bits of the B = 1 call on column c, under both rules.  Under STREAM with ONE inverse (w2) the groups
    of four (column, GP) vectors straddle the columns of the batch (35 vectors) and not those of a single column (7 vectors, 4 + 3)."""
    m = W.model(name)
    gm = device_model(G, m)
    B = W.WIDE[name]["B"]
    mu, cov, U, K = F.make_inputs(m, B)
    var = R.make_inputs(m, B)[1]
    diag, full = G.linearised_step(gm, mu, var, U, form=form), G.linearised_step_full(gm, mu, cov, U, K, form=form)
    for c in range(B):
        s = slice(c, c + 1)
        for k, (x, y) in enumerate(zip(diag + full, G.linearised_step(gm, mu[s], var[s], U[s], form=form) +
                                       G.linearised_step_full(gm, mu[s], cov[s], U[s], K, form=form))):
            assert same_bits(x[s], y), (c, ("mean", "variance", "Jacobian", "mean (full)", "Sigma'", "packed Jacobian")[k])


# ------------------------------------------------------------------------------------------------------------------ the rollouts
@functools.lru_cache(maxsize=None)
def reference_chain(name, full):
    """The long double chain of the case (shared by the two forms; not written to)."""
    m, pb = W.roll_model(name), W.problem(name)
    return F.chain(m, pb["x0"], pb["U"], pb["K"]) if full else R.rollout(m, pb["x0"], pb["U"])


def check_chain(G, gm, m, name, full, form, r, x0, U, K):
    """The rollout is the chain of step calls, bit for bit, and stays within the step bounds of the long double chain carried through |J|."""
    ds, da, B, H = W.dims_of(name)
    P0 = R.noise_model(m)[0]
    mu = torch.as_tensor(x0, device="cuda")
    st = torch.as_tensor(np.broadcast_to(P0 if full else np.diag(P0), (B, ds, ds) if full else (B, ds)).copy(), device="cuda")
    sk = "covs" if full else "vars"
    assert same_bits(r["means"][:, 0], mu) and same_bits(r[sk][:, 0], st)
    for t in range(H):
        Ut = U[:, t] if da else None
        if full:
            mu, st, jac = G.linearised_step_full(gm, mu, st, Ut, F.gain_at(K, t, ds, da), form=form)
        else:
            mu, st, jac = G.linearised_step(gm, mu, st, Ut, form=form)
        assert same_bits(r["means"][:, t + 1], mu) and same_bits(r[sk][:, t + 1], st) and same_bits(r["jac"][:, t], jac), t
    ref = reference_chain(name, full)
    means, state = r["means"].cpu().numpy(), r[sk].cpu().numpy()
    if full:
        HW._carried(ref["steps"], lambda s: f64(F.pack_state(TF.bounds(s)[0], TF.bounds(s)[1])), lambda s: s["jac"],
                    lambda t: F.pack_state(means[:, t], state[:, t]), lambda t: F.pack_state(ref["means"][:, t], ref["covs"][:, t]), B, F.packed_dim(ds))
    else:
        steps = [R.step(m, f64(ref["means"][:, t]), f64(ref["vars"][:, t]), U[:, t] if da else None) for t in range(H)]
        HW._carried(steps, lambda s: np.concatenate([TOL * f64(s["m_abs"]), TOL * f64(s["var_abs"]) + 4 * ULP * f64(s["var_mag"])], axis=1),
                    lambda s: s["jac"], lambda t: np.concatenate([means[:, t], state[:, t]], axis=1),
                    lambda t: np.concatenate([ref["means"][:, t], ref["vars"][:, t]], axis=1), B, 2 * ds)


@pytest.mark.parametrize("rule", ["diagonal", "full"])
@forms
@cases()
def test_rollout_chain_cost_gradient_constraints(G, name, form, rule):
    from gaussian_process_mpc_amd.rollout import rollout_constraints
    full = rule == "full"
    m = W.roll_model(name)
    gm = device_model(G, m)
    ds, da, B, H = W.dims_of(name)
    pb = W.problem(name)
    x0, U, K = pb["x0"], pb["U"], pb["K"]
    A, b, kappa = pb["rows"]
    sc = G.StateConstraints(A, b, kappa=kappa)
    rule_kw = dict(form=form, **(dict(full_covariance=True, feedback=K) if full else {}))
    sk = "covs" if full else "vars"
    if da == 0:
        # an autonomous model: the chain alone, and the refusals (what tests/test_host_model_frame.py and test_host_linprop_wide.py pin on
        # the C entries, here through the wrapper with a device present)
        assert U.shape == (B, H, 0) and K is None
        r = G.linearised_rollout(gm, x0, U, None, want_jac=True, **rule_kw)
        r2 = G.linearised_rollout(gm, x0, U, None, want_jac=True, chunk=64, **rule_kw)
        ro = G.linearised_rollout(gm, x0, U, None, want_grad=False, **rule_kw)
        for k in ("means", sk, "jac"):
            assert same_bits(r[k], r2[k]), k
        assert same_bits(ro["means"], r["means"]) and same_bits(ro[sk], r[sk]) and "jac" not in ro
        assert r["jac"].shape == ((B, H, 44, 44) if full else (B, H, 16, 16))
        check_chain(G, gm, m, name, full, form, r, x0, U, K)
        with pytest.raises(G.GpmpcError, match="a cost needs action_dim >= 1"):
            G.linearised_rollout(gm, x0, U, G.CostParams(0.5, np.eye(ds), np.zeros((0, 0))), want_grad=False, **rule_kw)
        # (objective only: with the gradient the wrapper's g_jac has H da = 0 columns, a NULL pointer, which the entries refuse first)
        with pytest.raises(G.GpmpcError, match="constraints need action_dim >= 1"):
            G.linearised_rollout(gm, x0, U, None, constraints=sc, want_grad=False, **rule_kw)
        with pytest.raises(ValueError, match="a feedback gain needs action_dim >= 1"):
            G.linearised_rollout(gm, x0, U, None, feedback=np.zeros((0, ds)), form=form)
        with pytest.raises(ValueError, match="a feedback gain needs action_dim >= 1"):
            G.linearised_step_full(gm, x0, np.tile(1e-2 * np.eye(ds), (B, 1, 1)), None, np.zeros((0, ds)), form=form)
        torch.cuda.synchronize()
        assert same_bits(G.linearised_rollout(gm, x0, U, None, want_jac=True, **rule_kw)["jac"], r["jac"])      # (and the library goes on)
        return
    cp, (gamma, Q, Rm), kw = TL.cost_case(G, m, H, np.random.default_rng(pb["cost_seed"]), W.WIDE[name].get("schedule", False))
    assert np.array_equal(Q, pb["Q"]) and np.array_equal(Rm, pb["R"])        # the draws the host file pins
    r = G.linearised_rollout(gm, x0, U, cp, want_jac=True, constraints=sc, **rule_kw)
    r2 = G.linearised_rollout(gm, x0, U, cp, want_jac=True, constraints=sc, chunk=64, **rule_kw)
    for k in ("means", sk, "jac", "cost", "grad", "g", "g_jac"):
        assert same_bits(r[k], r2[k]), k
    assert ("vars" in r) != full and r["g"].shape == (B, H, 3) and r["g_jac"].shape == (B, 3 * H, H * da)
    check_chain(G, gm, m, name, full, form, r, x0, U, K)
    # objective only: the same value bits, no Jacobians
    ro = G.linearised_rollout(gm, x0, U, cp, want_grad=False, constraints=sc, **rule_kw)
    assert same_bits(ro["means"], r["means"]) and same_bits(ro[sk], r[sk]) and same_bits(ro["cost"], r["cost"]) and same_bits(ro["g"], r["g"])
    assert "grad" not in ro and "g_jac" not in ro
    # cost and gradient: the long double adjoint on the returned arrays; gpmpc_cost_grad + the vjp entry within twice the bound
    Ud = torch.as_tensor(U, device="cuda")
    means, state, jacs = r["means"].cpu().numpy(), r[sk].cpu().numpy(), r["jac"].cpu().numpy()
    if full:
        ref = F.adjoint(jacs, means, state, U, gamma, Q, Rm, **kw)
        c_cg, g_vjp = TF.device_cost_grad_vjp(G, cp, r["means"], r["covs"], r["jac"], Ud)
    else:
        ref = R.adjoint(jacs, means, state, U, gamma, Q, Rm, **kw)
        c_cg, g_vjp = TL.device_cost_grad_vjp(G, cp, r["means"], r["vars"], r["jac"], Ud)
    A_c, A_g = f64(ref["A_cost"]), f64(ref["A_grad"])
    cost, grad = r["cost"].cpu().numpy(), r["grad"].cpu().numpy()
    w = {"cost": np.abs(cost - f64(ref["cost"])) / (TOL * A_c), "grad": np.abs(grad - f64(ref["grad"])) / (TOL * A_g),
         "cost vs gpmpc_cost_grad": np.abs(cost - c_cg.cpu().numpy()) / (2 * TOL * A_c),
         "grad vs cost_grad + vjp": np.abs(grad - g_vjp.cpu().numpy()) / (2 * TOL * A_g)}
    # constraints: the pure function on the returned arrays, bit for bit; the reference's forward sweep within its bound
    if full:
        rc = G.linearised_fc_constraints(r["means"], r["covs"], r["jac"], sc, ds, da)
        cref = F.constraints(means, state, jacs, A, b, kappa)
    else:
        rc = rollout_constraints(r["means"], r["vars"], r["jac"], sc, ds, da)
        cref = F.constraints(means, *W.embed_diag(state, jacs, ds, da), A, b, kappa)
    assert same_bits(rc["g"], r["g"]) and same_bits(rc["g_jac"], r["g_jac"])
    assert f64(cref["q"])[:, :, kappa > 0].min() >= HW.MIN_RADICAND          # no sd = 0 branch on the device's own trajectory either
    w["g"] = np.abs(r["g"].cpu().numpy() - f64(cref["g"])) / (TOL * f64(cref["A_g"]))
    Aj = TOL * f64(cref["A_gjac"])
    gj = r["g_jac"].cpu().numpy()
    assert np.all(gj[Aj == 0] == 0.0)
    w["g_jac"] = np.abs(gj - f64(cref["gjac"])) / np.where(Aj == 0, 1.0, Aj)
    print("  %s %s [%s]: of the bound: %s" % (name, rule, form, ", ".join("%s %.3g" % (k, float(v.max())) for k, v in w.items())))
    assert all(float(v.max()) <= 1.0 for v in w.values())
    for t in range(1, H + 1):                                                # causality: exact zeros, sign included
        blk = gj[:, (t - 1) * 3:t * 3, t * da:]
        assert not np.any(blk) and not np.any(np.signbit(blk)), t
    assert np.all(np.any(gj.reshape(B, H, 3, H, da)[:, H - 1, :, 0] != 0.0, axis=-1))    # the last step's rows do see the first input


# ------------------------------------------------------------------------------------------------------------------ the commanded input
@forms
@cases(W.INPUT_CASES)
def test_feedback_inputs(G, name, form):
    """input_cost and two input rows: cost, covariance seed, g_u and its Jacobian against feedback_inputs_reference on the returned arrays;
    means, covs, jac, g, g_jac keep the bits of the call without the options, which is the entry with nothing asked."""
    m = W.roll_model(name)
    gm = device_model(G, m)
    ds, da, B, H = W.dims_of(name)
    pb = W.problem(name, seed=W.INPUT_SEED)
    x0, U, K, C, d, kappa_u = pb["x0"], pb["U"], pb["K"], pb["C"], pb["d"], pb["kappa_u"]
    assert K.shape == (H, da, ds)
    cp, (gamma, Q, Rm), kw = TL.cost_case(G, m, H, np.random.default_rng(pb["cost_seed"]), W.WIDE[name].get("schedule", False))
    assert np.array_equal(Rm, pb["R"])
    sc = G.StateConstraints(*pb["rows"][:2], kappa=pb["rows"][2])
    ic = G.InputConstraints(C, d, kappa=kappa_u)
    base = dict(want_jac=True, constraints=sc, feedback=K, form=form)
    r = G.linearised_rollout(gm, x0, U, cp, input_cost=True, input_constraints=ic, **base)
    old = G.linearised_rollout(gm, x0, U, cp, **base)
    assert r["g_u"].shape == (B, H, 2) and r["g_u_jac"].shape == (B, 2 * H, H * da) and "g_u" not in old
    raw = TI.raw_rollout_inputs(G, gm, x0, U, K, cp, sc, True, form)
    for k in ("means", "covs", "jac", "cost", "grad", "g", "g_jac"):
        assert same_bits(raw[k], old[k]), k
    for k in ("means", "covs", "jac", "g", "g_jac"):
        assert same_bits(r[k], old[k]), k
    r64 = G.linearised_rollout(gm, x0, U, cp, input_cost=True, input_constraints=ic, chunk=64, **base)
    for k in r:
        assert same_bits(r[k], r64[k]), k
    ro = G.linearised_rollout(gm, x0, U, cp, want_grad=False, constraints=sc, feedback=K, form=form, input_cost=True, input_constraints=ic)
    assert same_bits(ro["cost"], r["cost"]) and same_bits(ro["g_u"], r["g_u"]) and same_bits(ro["g"], r["g"]) and same_bits(ro["covs"], r["covs"])
    assert "grad" not in ro and "g_u_jac" not in ro
    # the pure functions on the returned arrays, bit for bit
    Ud = torch.as_tensor(U, device="cuda")
    pc = G.feedback_input_cost(cp, r["covs"], K, da)
    assert same_bits(r["cost"], old["cost"] + pc["c"]), "out_cost is not cost_plain + c, one rounding"
    pu = G.feedback_input_constraints(Ud, r["covs"], r["jac"], ic, K)
    assert same_bits(pu["g_u"], r["g_u"]) and same_bits(pu["g_u_jac"], r["g_u_jac"])
    # against the long double reference on the returned arrays
    means, covs, jacs = r["means"].cpu().numpy(), r["covs"].cpu().numpy(), r["jac"].cpu().numpy()
    co, ru = I.input_cost(covs, K, Rm), I.input_constraints(U, covs, jacs, K, C, d, kappa_u)
    got = {"c": pc["c"].cpu().numpy(), "dcovs": pc["dcovs"].cpu().numpy(), "g": r["g_u"].cpu().numpy(), "gjac": r["g_u_jac"].cpu().numpy()}
    w = {"c": within(got["c"], co["c"], co["A_c"]), "seed": within(got["dcovs"], co["dcovs"], co["A_dcovs"]),
         "g_u": within(got["g"], ru["g"], ru["A_g"]), "g_u_jac": within(got["gjac"], ru["gjac"], ru["A_gjac"])}
    assert not np.any(got["dcovs"][:, H])
    ref = F.adjoint(jacs, means, covs, U, gamma, Q, Rm, **kw)
    gU = F.sweep(jacs, ref["dmu"], ref["dsig"] + co["dcovs"])[0]
    aU = F.sweep(np.abs(jacs), None, co["A_dcovs"])[0]
    tot = f64(ref["cost"] + co["c"])
    w["cost"] = float((np.abs(r["cost"].cpu().numpy() - tot) / (TOL * f64(ref["A_cost"] + co["A_c"]) + 4 * ULP * np.abs(tot))).max())
    dU = ref["grad"] - F.sweep(jacs, ref["dmu"], ref["dsig"])[0]              # the direct part of the reference gradient
    w["grad"] = float((np.abs(r["grad"].cpu().numpy() - f64(dU + gU)) / (TOL * f64(ref["A_grad"] + aU))).max())
    print("  %s [%s]: of the bound: %s" % (name, form, ", ".join("%s %.3g" % kv for kv in w.items())))
    assert max(w.values()) <= 1.0
    # causality: blocks tau > t are exact zeros, sign included; tau = t is c_rj
    gj = got["gjac"].reshape(B, H, 2, H, da)
    for t in range(H):
        assert not np.any(gj[:, t, :, t + 1:]) and not np.any(np.signbit(gj[:, t, :, t + 1:])), t
        assert np.array_equal(gj[:, t, :, t], np.broadcast_to(C, (B, 2, da))), t
    assert np.any(gj[:, H - 1, 0, 0] != 0.0) and np.any(gj[:, H - 1, 1, 0] != 0.0)
    for control in ["offdiag_once"] + ([W.INPUT_CONTROLS[name]] if name in W.INPUT_CONTROLS else []):
        miss = HW.input_control_miss(control, lambda k: got[k], co, ru, U, covs, jacs, K, Rm, C, d, kappa_u)
        print("  %s [%s]: the reference with %s misses by %.3g bounds" % (name, form, control, miss))
        assert miss >= 100.0


# ------------------------------------------------------------------------------------------------------------------ particles
@pytest.mark.parametrize("dims", W.PARTICLE_DIMS, ids=lambda d: "ds%d_da%d" % d)
def test_particle_step_with_three_inputs(G, dims):
    """k_pt_assemble and k_pt_finish at action_dim = 3: one step of B x P = 140 particles (three chunks of 64) against
    particle_reference.step, with the plan's inputs and with an input per particle; at (5, 3) the inputs themselves, v + K (x - mu)
    (k_lpi_pinputs), against the long double value.  Bounds: those of tests/test_gpu_particles.py and test_gpu_feedback_inputs.py."""
    ds, da = dims
    P, B, seed, call = W.PARTICLE_P, 2, 11, 2
    m = R.make_model(W.PARTICLE_N, ds, da, noise=True)
    gm = device_model(G, m)
    rng = np.random.default_rng(17)
    X, U_t = rng.uniform(-0.8, 0.8, (B, P, ds)), rng.uniform(-0.8, 0.8, (B, da))
    Kt, mu = rng.uniform(-0.5, 0.5, (da, ds)), rng.uniform(-0.8, 0.8, (B, ds))
    eps = G.particle_noise(P, da + ds, 1, seed, call)
    e = eps.cpu().numpy()
    assert np.abs(e - PR.normals(seed, call, 1, P, da + ds)).max() <= 1e-12
    s2_unit = 2.0 * ULP * (np.asarray(m["sf"]) ** 2 + PR.noise_model(m)[2])

    def worst(ref, nxt, mean):
        s2 = f64(ref["s2"])
        assert s2.min() > 0.0, "the reference clamps a particle: choose other inputs"
        tol = TOL * f64(ref["m_abs"]) + np.abs(e[None, :, da:]) * (TOL * f64(ref["q_abs"]) + s2_unit) / (2.0 * np.sqrt(s2)) + 4.0 * ULP * np.abs(f64(ref["next"]))
        return (float((np.abs(nxt.cpu().numpy() - f64(ref["next"])) / tol).max()),
                float((np.abs(mean.cpu().numpy() - f64(ref["m"])) / (TOL * f64(ref["m_abs"]))).max()))

    nxt, mean, var = G.particle_step(gm, X, U_t, eps, chunk=64, return_moments=True)
    again = G.particle_step(gm, X, U_t, eps, return_moments=True)
    assert all(same_bits(x, y) for x, y in zip((nxt, mean, var), again)), "chunk = 64 differs from the default"
    wp = worst(PR.step(m, X, U_t, e), nxt, mean)
    # an input per particle: u = v + K (x - mu), then the step at z = (x, u + sqrt(action_var) eps_u)
    Xd = torch.as_tensor(X, device="cuda")
    u = G.particle_inputs(Xd, U_t, Kt, mu)
    ref_u, A_u = I.particle_inputs(X, U_t, Kt, mu)
    wu = within(u.cpu().numpy(), ref_u, A_u)
    assert same_bits(G.particle_inputs(Xd, U_t), torch.as_tensor(U_t, device="cuda")[:, None].expand(B, P, da).contiguous())
    nxt_u, mean_u, _ = G.particle_step_inputs(gm, Xd, u, eps, chunk=64)
    assert all(same_bits(x, y) for x, y in zip((nxt_u, mean_u), G.particle_step_inputs(gm, Xd, u, eps)[:2]))
    z = np.concatenate([X, u.cpu().numpy() + np.sqrt(PR.noise_model(m)[1])[None, None, :] * e[None, :, :da]], axis=-1)
    ref = {k: v.reshape(B, P, ds) for k, v in PR.posterior(m, z.reshape(-1, ds + da)).items()}
    ref["next"] = ref["m"] + PR._sqrt(ref["s2"]) * R.G.cast(e[:, da:])[None]
    wq = worst(ref, nxt_u, mean_u)
    print("  particles ds %d da %d: the plan's inputs: draw %.3g, mean %.3g; inputs v + K (x - mu) %.3g; an input per particle: draw %.3g, "
          "mean %.3g of the bound" % ((ds, da) + wp + (wu,) + wq))
    assert max(wp + (wu,) + wq) <= 1.0
    assert not same_bits(nxt, nxt_u)                                         # (the per-particle inputs did reach the step)
