"""GPU tests of the STREAM form of the linearised step (csrc/linprop_stream.hip; include/gpmpc.h, "Linearised propagation") and of the
choice between the forms.  The references, cases, bounds and test bodies are those of tests/test_gpu_linprop.py, run with STREAM selected by
a module fixture: no tolerance is new.

Boundaries of the STREAM kernels and the case that crosses each: the 32-row block and the 8 rows of a wave (n = 64, 70, 130); the 128-column
chunk of a row, with the prefetch of the next one (n = 130: two chunks); the group of GPMPC_LINPROP_STREAM_COLS vectors and the 16 columns
of a set of launches (case b, B = 65, one matrix: groups of (column, GP) pairs; B = COLS + 1 with a matrix per GP); the 256-row block of the
k / gradient kernels, which n = 64, 70, 130 do NOT cross: case g, n = 257, the smallest n that does (two blocks, the second with one live
row and with threads beyond the padded length).  n = 257 is odd as well: its rows are not 16-byte aligned, so it runs the 8-byte loads."""
import numpy as np
import pytest
import torch

import linprop_reference as R
import test_gpu_linprop as T

pytestmark = pytest.mark.gpu
same_bits = T.same_bits
f64 = T.f64


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    return g


@pytest.fixture(scope="module", autouse=True)
def stream(G):
    """STREAM for the whole module; the form found before it is restored, and yielded."""
    from gaussian_process_mpc_amd import _lib
    old = _lib.lib().gpmpc_linearised_set_form(_lib.LINPROP_FORM_STREAM)
    yield old
    assert _lib.lib().gpmpc_linearised_set_form(old) == _lib.LINPROP_FORM_STREAM


def selected():
    from gaussian_process_mpc_amd import _lib
    return _lib.lib().gpmpc_linearised_set_form(-1)


CASE_G = dict(n=257, ds=2, da=1, B=5)


def model_g():
    return R.make_model(CASE_G["n"], CASE_G["ds"], CASE_G["da"])


# ------------------------------------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_step_against_reference(G, name):
    assert selected() == 1
    T.test_step_against_reference(G, name)


def test_step_nonsymmetric_inverse(G):
    T.test_step_nonsymmetric_inverse(G)


def test_step_sparse_model(G):
    T.test_step_sparse_model(G)


def test_step_across_the_256_row_block(G):
    """Case g: n = 257 (see the module docstring)."""
    m = model_g()
    T.check_step(G, T.device_model(G, m), m, CASE_G["B"], "case g (n = 257)", control="drop_h")


# ------------------------------------------------------------------------------------------------------------------ columns
@pytest.mark.parametrize("name", ["a", "d", "b"])
def test_columns_are_independent(G, name):
    """Column c of a batch of COLS + 1 has the bits of the B = 1 call on column c (case b: one matrix, groups of (column, GP) pairs)."""
    from gaussian_process_mpc_amd import _lib
    m = T.case_model(name)
    gm = T.device_model(G, m)
    B = _lib.LINPROP_STREAM_COLS + 1
    mu, var, U = R.make_inputs(m, B)
    full = G.linearised_step(gm, mu, var, U)
    again = G.linearised_step(gm, mu, var, U)
    assert all(same_bits(x, y) for x, y in zip(full, again)), "two identical calls differ"
    for c in range(B):
        one = G.linearised_step(gm, mu[c:c + 1], var[c:c + 1], U[c:c + 1])
        for k, (x, y) in enumerate(zip(full, one)):
            assert same_bits(x[c:c + 1], y), (c, ("mean", "variance", "Jacobian")[k])


# ------------------------------------------------------------------------------------------------------------------ the rollout, MPPI
@pytest.mark.parametrize("name,schedule", [("a", False), ("c", False), ("d", True)])
def test_rollout_chain_cost_gradient_constraints(G, name, schedule):
    assert selected() == 1
    T.test_rollout_chain_cost_gradient_constraints(G, name, schedule)


@pytest.mark.parametrize("constrained", [False, True])
def test_mppi_solve_linearised_is_the_host_loop(G, constrained):
    """K = 8: the C entry reaches the step through the rollout, the host loop through ``linearised_rollout``: one dispatcher."""
    assert selected() == 1
    T.test_mppi_solve_linearised_is_the_host_loop(G, constrained)


# ------------------------------------------------------------------------------------------------------------------ the choice
def _three(G, gm, mu, var, U):
    return {f: G.linearised_step(gm, mu, var, U, form=f) for f in ("tile", "stream", "auto")}


def test_auto_is_the_form_it_picked(G):
    from gaussian_process_mpc_amd import _lib
    m = T.case_model("a")
    gm = T.device_model(G, m)
    MAXB = _lib.LINPROP_AUTO_MAX_B
    for B, want in ((max(MAXB, 1), "stream" if MAXB >= 1 else "tile"), (MAXB + 1, "tile")):
        o = _three(G, gm, *R.make_inputs(m, B))
        assert all(same_bits(x, y) for x, y in zip(o["auto"], o[want])), (B, want)
        other = "tile" if want == "stream" else "stream"
        assert not all(same_bits(x, y) for x, y in zip(o["auto"], o[other])), (B, other)      # (the two forms do differ in bits here)
    # the rollout goes through the same dispatcher
    B, H = MAXB + 1, 2
    rng = np.random.default_rng(3)
    x0, U = rng.uniform(-1, 1, (B, 2)), rng.uniform(-1, 1, (B, H, 1))
    ra, rt = G.linearised_rollout(gm, x0, U, form="auto"), G.linearised_rollout(gm, x0, U, form="tile")
    assert same_bits(ra["means"], rt["means"]) and same_bits(ra["vars"], rt["vars"])
    assert selected() == 1                               # form= restored the module's choice


def test_untouched_default_is_tile(G, stream):
    from gaussian_process_mpc_amd import _lib
    L = _lib.lib()
    assert stream == _lib.LINPROP_FORM_DEFAULT == _lib.LINPROP_FORM_TILE
    m = T.case_model("a")
    gm = T.device_model(G, m)
    mu, var, U = R.make_inputs(m, 3)
    explicit = G.linearised_step(gm, mu, var, U, form="tile")
    L.gpmpc_linearised_set_form(stream)
    try:
        default = G.linearised_step(gm, mu, var, U)
    finally:
        L.gpmpc_linearised_set_form(_lib.LINPROP_FORM_STREAM)
    assert all(same_bits(x, y) for x, y in zip(default, explicit))


def test_stream_against_tile(G):
    """Both forms are within their bounds of the long double reference on case a, hence within twice the bound of each other."""
    m = T.case_model("a")
    gm = T.device_model(G, m)
    mu, var, U = R.make_inputs(m, T.CASES["a"]["B"])
    ref = R.step(m, mu, var, U)
    o = {f: [t.cpu().numpy() for t in G.linearised_step(gm, mu, var, U, form=f)] for f in ("tile", "stream")}
    for f in o:
        w = T.worst_step(ref, *o[f])
        print("  %s: mean %.3f, var %.3f, Jacobian %.3f of the bound" % ((f,) + w))
        assert max(w) <= 1.0
    bm = T.TOL * f64(ref["m_abs"])
    bv = T.TOL * f64(ref["var_abs"]) + 4 * T.ULP * f64(ref["var_mag"])
    bj = T.TOL * f64(ref["jac_abs"]) + 4 * T.ULP * f64(ref["jac_mag"])
    for k, b in enumerate((bm, bv, bj)):
        d = np.abs(o["tile"][k] - o["stream"][k])
        print("  tile vs stream, output %d: worst %.3f of twice the bound" % (k, float((d / np.where(b == 0, 1.0, 2 * b)).max())))
        assert np.all(d <= 2.0 * b)


# ------------------------------------------------------------------------------------------------------------------ RiskSensitiveMPC
def test_mpc_linearised_form(G, stream):
    from gaussian_process_mpc_amd import _lib
    L = _lib.lib()
    mpc, pb = T._mpc(G)
    H = mpc.horizon
    U = np.ascontiguousarray(pb["U"][:, :H])
    x = U[0].reshape(-1)
    mpc.set_state_constraints(np.array([[1.0, 0.0]]), [0.4], prob=0.9)
    mpc.propagation = "linearised"
    assert mpc.linearised_form is None
    L.gpmpc_linearised_set_form(stream)                  # the process as the parent leaves it: TILE, nothing selected
    try:
        before = selected()
        kw = dict(constraints=mpc.state_constraints)
        # None: the bits of the parent's path, explicit TILE
        rt = G.linearised_rollout(mpc.dynamics, mpc.curr_state, U[:1], mpc._cost_params(), form="tile", **kw)
        assert mpc.objective(x) == rt["cost"][0].item()
        assert np.array_equal(np.asarray(mpc.gradient(x)), rt["grad"][0].cpu().numpy())
        assert np.array_equal(np.asarray(mpc.constraints(x)), rt["g"][0].cpu().numpy().reshape(-1))
        assert np.array_equal(np.asarray(mpc.jacobian(x)), rt["g_jac"][0].cpu().numpy().reshape(-1))
        # "stream": the four callbacks at one x are linearised_rollout(form="stream") at B = 1; evaluate_batch matches
        mpc.linearised_form = "stream"
        x2 = U[1].reshape(-1)                            # (another x: the callbacks cache their last evaluation)
        rs = G.linearised_rollout(mpc.dynamics, mpc.curr_state, U[1:2], mpc._cost_params(), form="stream", **kw)
        assert mpc.objective(x2) == rs["cost"][0].item()
        assert np.array_equal(np.asarray(mpc.gradient(x2)), rs["grad"][0].cpu().numpy())
        assert np.array_equal(np.asarray(mpc.constraints(x2)), rs["g"][0].cpu().numpy().reshape(-1))
        assert np.array_equal(np.asarray(mpc.jacobian(x2)), rs["g_jac"][0].cpu().numpy().reshape(-1))
        rb = G.linearised_rollout(mpc.dynamics, mpc.curr_state, U, mpc._cost_params(), form="stream", **kw)
        eb = mpc.evaluate_batch(U, constraints=True)
        for k in ("cost", "grad", "means", "vars", "g", "g_jac"):
            assert same_bits(eb[k], rb[k]), k
        assert same_bits(eb["cost"][1:2], rs["cost"])
        rbt = G.linearised_rollout(mpc.dynamics, mpc.curr_state, U, mpc._cost_params(), form="tile", **kw)
        assert not same_bits(rb["vars"], rbt["vars"])    # (so the comparison above does tell the forms apart)
        v = mpc.validate_plan(U=U[0], x0=pb["x0"][0], particles=256, seed=0, linearised=True)
        ln = G.linearised_rollout(mpc.dynamics, pb["x0"][0], U[0], None, want_grad=False, form="stream")
        assert np.array_equal(v["var_lin"], ln["vars"][0].cpu().numpy())
        # the solvers that take it
        mpc.mppi_options.update(samples=16, iterations=3)
        plan = mpc.get_optimal_trajectory(pb["x0"][0], solver="mppi")
        assert plan.shape == (H, 1) and np.all(np.isfinite(plan)) and np.isfinite(mpc.last_solve_info["cost"])
        mpc.clear_state_constraints()
        mpc.multistart_options.update(max_ticks=3)
        plan = mpc.get_optimal_trajectory(pb["x0"][0], n_starts=2)
        assert plan.shape == (H, 1) and np.all(np.isfinite(plan)) and mpc.solver_used == "lockstep-lbfgs x2"
        assert selected() == before                      # the process-wide form is what it was
    finally:
        L.gpmpc_linearised_set_form(_lib.LINPROP_FORM_STREAM)
