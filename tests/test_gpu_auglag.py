"""GPU tests of the constrained multi-start: k_al_merit / k_al_outer / k_al_finish (csrc/auglag.hip) against the numpy
restatement of tests/auglag_reference.py on hand-made inputs, batch independence, gpmpc_auglag_solve against its parts, the solve on c1, and
solver="auglag" of RiskSensitiveMPC open and closed loop.

Tolerance of the parities (tests 1 and 2): the protocol of tests/test_gpu_lbfgs.py.  The restatement is evaluated on the same inputs in float64
and in np.longdouble on the CPU; the tolerance of a floating-point field is 8 x the largest relative difference seen between the two (over
all fields of the case, each relative to the largest magnitude of its field), scaled by the largest magnitude of that field, with a floor of
1e-13.  Flags and counters are compared exactly, copies bit for bit, and every inequality of the rule that compares computed quantities is
asserted to have a relative margin of at least 1e-6 on the inputs used.  Every case prints its own figures; the maxima measured on an MI355X
are in the docstrings of the tests."""
import ctypes

import numpy as np
import pytest
import torch

import auglag_reference as AR
from constraints_reference import reference_constraints, reference_cost
from nominal_reference import synth_nominal

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
K95 = 1.6448536269514722
SLSQP = {0.1: 1.86235, 0.3: 1.87492}                         # tests/test_gpu_constraints.py::test_constrained_solve
SHAPES = [(1, 1), (1, 3), (10, 2), (13, 5), (65, 2)]         # (H, da): one column, a partial wave, 20, 65 and 130 columns


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    return g


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)).view(np.uint64)


def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def _fin(a):
    return np.where(np.isfinite(np.asarray(a, dtype=np.float64)), a, 0.0)


def _protocol(fields):
    """fields: name -> (float64 restatement, longdouble restatement, device).  Asserts the protocol, returns (rel, worst)."""
    rel = 0.0
    for a64, ald, _ in fields.values():
        scale = np.abs(_fin(a64)).max() if np.size(a64) else 0.0
        if scale > 0:
            rel = max(rel, float(np.abs(_fin(ald) - _fin(a64).astype(np.longdouble)).max() / scale))
    worst = 0.0
    for f, (a64, _, dev) in fields.items():
        np.testing.assert_array_equal(np.isfinite(a64), np.isfinite(dev), err_msg=f)
        scale = np.abs(_fin(a64)).max() if np.size(a64) else 0.0
        tol = max(8.0 * rel * scale, 1e-13)
        err = float(np.abs(_fin(dev) - _fin(a64)).max()) if np.size(a64) else 0.0
        worst = max(worst, err / max(scale, 1e-300))
        assert err <= tol, (f, err, tol, rel)
    return rel, worst


# ------------------------------------------------------------------------------------------------------------------------------
# 1. merit
# ------------------------------------------------------------------------------------------------------------------------------
def _merit_inputs(K, H, da, mc, seed, special=True):
    """Hand-made (f, grad, g, g_jac, lam, rho): rows active and inactive, none within 1e-6 (relative) of the switch; the g_jac row of an
    inactive row is NaN.  With ``special`` and K >= 5: start 1 has a NaN in g, start 3 has f = +inf."""
    rng = np.random.default_rng(seed)
    n, R = H * da, H * mc
    f = rng.uniform(1.0, 2.0, K)
    grad = rng.uniform(-1.0, 1.0, (K, n))
    g = rng.uniform(0.05, 1.0, (K, R)) * rng.choice([-1.0, 1.0], (K, R))
    lam = rng.uniform(0.1, 2.0, (K, R)) * (rng.uniform(size=(K, R)) < 0.6)
    rho = rng.choice([0.5, 10.0, 100.0], K)
    if R >= 2:                                               # every start has an active and an inactive row
        g[:, 0], lam[:, 0] = 0.5, 0.25
        g[:, 1], lam[:, 1] = -0.75, 0.0
    t = lam + rho[:, None] * g
    margin = (np.abs(t) / np.maximum(np.abs(lam), np.abs(rho[:, None] * g))).min()
    g_jac = rng.uniform(-1.0, 1.0, (K, R, n))
    g_jac[t <= 0] = NAN
    bad = []
    if special and K >= 5:
        g[1, R // 2] = NAN
        f[3] = INF
        bad = [1, 3]
    return (f, grad, g, g_jac, lam, rho), margin, (t > 0), bad


def _device_merit(inp, K, H, da, mc):
    from gaussian_process_mpc_amd.device_auglag import auglag_merit
    f, grad, g, g_jac, lam, rho = inp
    M, dM = auglag_merit(f, grad.reshape(K, H, da), g.reshape(K, H, mc), g_jac, lam, rho)
    return M.cpu().numpy(), dM.cpu().numpy().reshape(K, H * da)


@pytest.mark.parametrize("mc", [1, 3, 16])
@pytest.mark.parametrize("H,da", SHAPES)
@pytest.mark.parametrize("K", [1, 5, 64])
def test_merit_matches_the_restatement(G, K, H, da, mc):
    """k_al_merit on hand-made inputs against the restatement.  Measured on an MI355X over the 45 cases: float64 against longdouble at
    most 1.8e-15 relative (K = 1, n = 130, R = 1040), so the tolerance is the floor of 1e-13 but for fields of magnitude above 7; device
    against restatement at most 6.7e-16 relative (K = 5, n = 130, R = 1040); the smallest margin of the switch t_i = 0 is 2.1e-4."""
    seed = 10000 * mc + 100 * (H * da) + K
    inp, margin, active, bad = _merit_inputs(K, H, da, mc, seed)
    assert margin >= 1e-6
    if H * mc >= 2:
        assert active.any(axis=1).all() and (~active).any(axis=1).all()
    good = np.array([k for k in range(K) if k not in bad], dtype=int)
    M64, dM64 = AR.merit(*inp)
    with np.errstate(invalid="ignore"):
        Mld, dMld = AR.merit(*[_ld(a) for a in inp])
    M, dM = _device_merit(inp, K, H, da, mc)
    assert np.isfinite(dM[good]).all()                       # the NaN rows of g_jac were not read
    for k in bad:
        assert not np.isfinite(M[k]) and not np.isfinite(M64[k])
    rel, worst = _protocol({"M": (M64[good], Mld[good], M[good]), "dM": (dM64[good], dMld[good], dM[good])})
    print("K = %d, n = %d, R = %d: float64 vs longdouble %.2e relative, device vs restatement %.2e relative (allowed %.2e), smallest margin "
          "%.1e" % (K, H * da, H * mc, rel, worst, max(8 * rel, 1e-13), margin))
    if bad:                                                  # the other starts do not notice the two bad ones
        clean, _, _, _ = _merit_inputs(K, H, da, mc, seed, special=False)
        M2, dM2 = _device_merit(clean, K, H, da, mc)
        assert np.isfinite(M2).all()
        np.testing.assert_array_equal(_bits(M[good]), _bits(M2[good]))
        np.testing.assert_array_equal(_bits(dM[good]), _bits(dM2[good]))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. outer step
# ------------------------------------------------------------------------------------------------------------------------------
RULE = dict(growth=10.0, shrink=0.25, rho_max=1e3, lam_max=50.0, feas_tol=1e-4)
SCENARIOS = ("grow", "nogrow", "cap", "lam_hi", "lam_lo", "settle", "replace", "keep", "feas_beats", "tie_replace", "tie_keep", "dead_f",
             "dead_g", "unconverged")
FLOATS = ("rho", "V_prev", "lam")
COPIES = ("v", "f", "inc_v", "inc_f", "inc_x")


def _outer_inputs(K, H, da, mc, seed):
    """K states and the evaluation (f, g) of the points X, start k built for SCENARIOS[(k + seed) % len]."""
    rng = np.random.default_rng(seed)
    n, R = H * da, H * mc
    kind = [SCENARIOS[(k + seed) % len(SCENARIOS)] for k in range(K)]
    X = rng.uniform(-1, 1, (K, n))
    st = AR.new_state(rng.uniform(-1, 1, (K, n)), R, rho0=10.0)
    st["lam"] = rng.uniform(0.5, 2.0, (K, R))
    f = rng.uniform(1.0, 2.0, K)
    g = rng.uniform(0.1, 0.5, (K, R)) * rng.choice([-1.0, 1.0], (K, R))
    g[:, 0] = 0.45                                           # (some row is violated unless the scenario says otherwise)
    st["inc_v"], st["inc_f"] = np.full(K, 0.9), rng.uniform(1.0, 2.0, K)          # default: replaced (0.5 < 0.9)
    conv = np.ones(K)
    for k, sc in enumerate(kind):
        if sc == "cap":
            st["rho"][k] = 500.0
        if sc == "lam_hi":
            st["lam"][k, 0] = 48.0                           # 48 + 10 * 0.45 > 50
        if sc in ("lam_lo", "feas_beats", "tie_replace", "tie_keep"):
            g[k] = -np.abs(g[k])
        if sc in ("settle", "unconverged"):
            g[k], st["lam"][k] = -np.abs(g[k]), 0.0          # V = 0
            conv[k] = 0.0 if sc == "unconverged" else 1.0
        if sc == "keep":
            st["inc_v"][k], st["inc_f"][k] = 0.0, 5.0        # feasible and dearer: an infeasible point does not replace it
        if sc == "feas_beats":
            st["inc_v"][k], st["inc_f"][k] = 0.3, 0.1        # infeasible and cheaper: a feasible point replaces it
        if sc == "tie_replace":
            st["inc_v"][k], st["inc_f"][k] = 0.0, 2.5
        if sc == "tie_keep":
            st["inc_v"][k], st["inc_f"][k] = 0.0, 0.5
        if sc == "dead_f":
            f[k] = NAN
        if sc == "dead_g":
            g[k, R - 1] = -INF
    # V_prev from the V this step will see: grow where V > shrink V_prev
    with np.errstate(invalid="ignore"):
        V = np.abs(np.maximum(g, -st["lam"] / st["rho"][:, None])).max(axis=1)
    st["V_prev"] = np.where([sc == "nogrow" for sc in kind], 8.0 * V, V)
    st["settled"] = rng.uniform(size=K) < 0.5
    return st, f, g, X, conv, kind


def _device_outer(st, f, g, X, conv, alive, K, H, da, mc, update):
    from gaussian_process_mpc_amd.device_auglag import auglag_outer, auglag_state_fields, auglag_state_layout, auglag_state_view
    state = torch.zeros(auglag_state_layout(K, H * da, H * mc)["total"], dtype=torch.float64)
    v = auglag_state_view(state, K, H, da, mc)
    for name in ("rho", "V_prev", "v", "f", "inc_v", "inc_f", "lam", "inc_x", "alive", "settled"):
        v[name].copy_(torch.from_numpy(np.asarray(st[name], dtype=np.float64).reshape(tuple(v[name].shape))))
    before = state.cuda()
    after = auglag_outer(before.clone(), f, g.reshape(K, H, mc), X.reshape(K, H, da), K, H, da, update=update, conv=conv, alive=alive,
                         lb=-1.0, ub=1.0, **RULE)
    return before, after, auglag_state_fields(after, K, H, da, mc)


def _outer_margins(rep, st, g):
    worst = INF

    def take(lhs, rhs):
        nonlocal worst
        lhs, rhs = np.asarray(lhs, dtype=np.float64), np.broadcast_to(np.asarray(rhs, dtype=np.float64), np.shape(lhs))
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.abs(lhs - rhs) / np.maximum(np.abs(lhs), np.abs(rhs))
        r = r[np.isfinite(r)]
        if len(r):
            worst = min(worst, r.min())
    i, v, tol = rep["feasible"]
    take(v, tol)
    _, kv, iv, fi, ic, _ = rep["key"]
    take(kv[kv != iv], iv[kv != iv])
    take(fi[kv == iv], ic[kv == iv])
    if "lam" in rep:
        _, t, cap = rep["lam"]
        take(t, 0.0)
        take(t, cap)
        _, V, bound, _ = rep["grow"]
        take(V, bound)
        take(rep["cap"][1], rep["cap"][2])
        take(rep["settle"][1], rep["settle"][2])
        take(g[i], -st["lam"][i] / st["rho"][i][:, None])
    assert worst >= 1e-6, worst
    return worst


@pytest.mark.parametrize("update", [True, False])
@pytest.mark.parametrize("H,da,mc", [(1, 1, 1), (10, 2, 1), (13, 5, 3), (65, 2, 16)])
@pytest.mark.parametrize("K", [1, 5, 64])
def test_outer_step_matches_the_restatement(G, K, H, da, mc, update):
    """k_al_outer and k_al_finish on hand-made states against the restatement.  Measured on an MI355X over the 24 cases:
    float64 against longdouble at most 4.1e-17 relative (one multiply and one add per element), device against restatement 0 (every field
    bit for bit); the smallest margin of an inequality is 5.1e-5."""
    from gaussian_process_mpc_amd.device_auglag import auglag_state_view
    seed = 1000 * mc + 10 * H * da + K
    st, f, g, X, conv, kind = _outer_inputs(K, H, da, mc, seed)
    alive = (np.arange(K) % 5 != 4).astype(np.float64)
    ref, rep = AR.outer(st, f, g, X, conv, update, want_report=True, **RULE)
    with np.errstate(invalid="ignore"):
        ref_ld = AR.outer({k: (_ld(v) if np.asarray(v).dtype == np.float64 else v) for k, v in st.items()}, _ld(f), _ld(g), _ld(X), conv, update,
                          **RULE)
    margin = _outer_margins(rep, st, g) if not rep["dead"].all() else INF
    # what was built is what the restatement took
    for k, sc in enumerate(kind):
        replaced = not np.array_equal(ref["inc_x"][k], st["inc_x"][k])
        assert replaced == (sc not in ("keep", "tie_keep", "dead_f", "dead_g")), (k, sc)
        if sc in ("dead_f", "dead_g"):
            assert rep["dead"][k]
        if not update:
            continue
        if sc in ("grow", "lam_hi", "replace", "keep"):
            assert ref["rho"][k] == 100.0
        if sc == "nogrow":
            assert ref["rho"][k] == 10.0
        if sc == "cap":
            assert ref["rho"][k] == 1000.0
        if sc == "lam_hi":
            assert ref["lam"][k, 0] == 50.0
        if sc == "lam_lo":
            assert (ref["lam"][k] == 0.0).any() and (ref["lam"][k] >= 0.0).all()
        if sc in ("settle", "unconverged"):
            assert ref["settled"][k] == (sc == "settle") and ref["V_prev"][k] == 0.0
    before, after, got = _device_outer(st, f, g, X, conv, alive, K, H, da, mc, update)
    best, key, open_ = AR.finish(ref, alive)
    np.testing.assert_array_equal(got["settled"], ref["settled"])
    np.testing.assert_array_equal(got["alive"], alive != 0.0)
    assert (got["not_settled"], got["best"], got["best_v"], got["best_f"]) == (open_, best, key[0], key[1])
    np.testing.assert_array_equal(_bits(got["plan"]), _bits(got["inc_x"][best]))
    for name in COPIES:                                      # maxima, selects and copies: exact
        np.testing.assert_array_equal(_bits(got[name]), _bits(ref[name]), err_msg=name)
    rel, worst = _protocol({name: (ref[name], np.asarray(ref_ld[name]), got[name]) for name in FLOATS})
    print("K = %d, n = %d, R = %d, update %d: float64 vs longdouble %.2e relative, device vs restatement %.2e relative (allowed %.2e), smallest "
          "margin %.1e" % (K, H * da, H * mc, update, rel, worst, max(8 * rel, 1e-13), margin))
    vb, va = auglag_state_view(before, K, H, da, mc), auglag_state_view(after, K, H, da, mc)
    for k, sc in enumerate(kind):                            # a dead start is left bit for bit as it is
        if sc in ("dead_f", "dead_g"):
            for name in ("rho", "V_prev", "v", "f", "inc_v", "inc_f", "settled", "lam", "inc_x"):
                np.testing.assert_array_equal(_bits(va[name][k]), _bits(vb[name][k]), err_msg=name)
    if not update:                                           # incumbents only
        for name in ("rho", "V_prev", "settled", "lam"):
            np.testing.assert_array_equal(_bits(va[name]), _bits(vb[name]), err_msg=name)
    if K == 64:
        assert set(kind) == set(SCENARIOS)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. batch independence
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,da,mc", [(10, 2, 3), (65, 2, 16)])
def test_batch_independence_and_reproducibility(G, H, da, mc):
    from gaussian_process_mpc_amd.device_auglag import auglag_state_view
    K = 64
    inp, _, _, _ = _merit_inputs(K, H, da, mc, 7)
    M, dM = _device_merit(inp, K, H, da, mc)
    M2, dM2 = _device_merit(inp, K, H, da, mc)
    np.testing.assert_array_equal(_bits(M), _bits(M2))
    np.testing.assert_array_equal(_bits(dM), _bits(dM2))
    st, f, g, X, conv, kind = _outer_inputs(K, H, da, mc, 7)
    _, a, _ = _device_outer(st, f, g, X, conv, None, K, H, da, mc, True)
    _, b, _ = _device_outer(st, f, g, X, conv, None, K, H, da, mc, True)
    np.testing.assert_array_equal(_bits(a), _bits(b))        # two identical calls: the whole buffer
    va = auglag_state_view(a, K, H, da, mc)
    for k in range(K):
        M1, dM1 = _device_merit(tuple(x[k:k + 1] for x in inp), 1, H, da, mc)
        np.testing.assert_array_equal(_bits(M1[0]), _bits(M[k]))
        np.testing.assert_array_equal(_bits(dM1[0]), _bits(dM[k]))
        one = {name: v[k:k + 1] for name, v in st.items()}
        _, s1, _ = _device_outer(one, f[k:k + 1], g[k:k + 1], X[k:k + 1], conv[k:k + 1], None, 1, H, da, mc, True)
        v1 = auglag_state_view(s1, 1, H, da, mc)
        for name in ("rho", "V_prev", "v", "f", "inc_v", "inc_f", "alive", "settled", "lam", "inc_x"):
            np.testing.assert_array_equal(_bits(v1[name][0]), _bits(va[name][k]), err_msg="%s of start %d (%s)" % (name, k, kind[k]))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. / 5. on c1
# ------------------------------------------------------------------------------------------------------------------------------
_c1 = {}


def _mpc_c1(G):
    from oracle import gpmpc_oracle as O
    from gaussian_process_mpc_amd.synth import synth_problem
    pb = synth_problem(1, 100, 2, 2, 10, 64)
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    mpc = G.RiskSensitiveMPC(1e-5, H, ds, da, pb["Q"], pb["R"])
    for a, g in enumerate(mpc.dynamics.gpr_err):
        g.set_lambdas(pb["lambdas"][a])
        g.set_sigma_n(float(pb["sigma_n"][a]))
        g.set_sigma_f(1.0)
    mpc.dynamics.append_train_data(pb["X"][:, :ds], pb["X"][:, ds:], pb["Y"])
    Kinv = torch.stack([g.Ky_inv.detach().cpu() for g in mpc.dynamics.gpr_err])
    gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"], Ky_inv=Kinv)
    mpc.set_lb([-1.0] * da)
    mpc.set_ub([1.0] * da)
    return mpc, gp, pb


def _problem(G):
    """c1, trajectory 0, and the construction of tests/test_gpu_constraints.py::test_constrained_solve: one 95 % row on state 0,
    b(f) = top - f span of mu_t0 + kappa sd_t0 along the unconstrained optimum of the default solver from the zero start."""
    if not _c1:
        from gaussian_process_mpc_amd.multistart import make_starts
        mpc, gp, pb = _mpc_c1(G)
        H, x0 = pb["H"], pb["x0"][0]
        n = H * pb["da"]
        U_free = mpc.get_optimal_trajectory(x0)
        A = np.array([[1.0, 0.0]])
        along = reference_constraints(gp, H, x0, U_free, A, [0.0], [K95], want_jac=False)["g"][:, 0]
        top, span = along.max(), along.max() - along.min()
        X0 = make_starts(4, n, np.full(n, -1.0), np.full(n, 1.0), np.random.default_rng([0, 0]))
        assert not X0[0].any()
        _c1.update(mpc=mpc, gp=gp, pb=pb, A=A, b={f: top - f * span for f in SLSQP}, X0=X0, U_free=U_free, used=mpc.solver_used)
    return _c1


def _pack(G, nominal=False):
    c = _problem(G)
    pb, gp = c["pb"], c["gp"]
    return G.GPPack(pb["X"], pb["Y"], gp.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"], nominal=synth_nominal(2, 2) if nominal else None)


def _cost(G):
    pb = _problem(G)["pb"]
    return G.CostParams(1e-5, pb["Q"], pb["R"], x_ref=pb["x_ref"], u_ref=pb["u_ref"])


def _sc(G, f=0.3):
    c = _problem(G)
    return G.StateConstraints(c["A"], [c["b"][f]], prob=0.95)


def _log_into(log):
    def callback(done, ws, inner_offset):
        log.append((done, ws.clone(), inner_offset))
    return callback


def test_solve_equals_its_parts_bit_for_bit(G):
    from gaussian_process_mpc_amd.device_auglag import auglag_merit, auglag_outer, auglag_solve, auglag_state_layout, auglag_state_new, auglag_state_view
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_start, lbfgs_state_layout, lbfgs_state_view, lbfgs_tick
    c = _problem(G)
    pb, X0 = c["pb"], c["X0"]
    pack, cost, sc = _pack(G), _cost(G), _sc(G)
    H, da, x0, K, m, T, NO = pb["H"], pb["da"], pb["x0"][0], 4, 8, 5, 3
    n = H * da
    ta, tl = auglag_state_layout(K, n, H * sc.m)["total"], lbfgs_state_layout(K, n, m)["total"]
    lkw = dict(lb=-1.0, ub=1.0, history=m, gtol=1e-6, ftol=1e-12)
    one, two = [], []
    U1, c1, info1 = auglag_solve(pack, x0, X0.reshape(K, H, da), cost, sc, outer=NO, inner_ticks=T, check_outer=0, callback=_log_into(one), **lkw)
    U2, c2, info2 = auglag_solve(pack, x0, X0.reshape(K, H, da), cost, sc, outer=NO, inner_ticks=T, check_outer=2, callback=_log_into(two), **lkw)
    assert [d for d, _, _ in one] == [NO] and [d for d, _, _ in two] == [2, NO] and one[0][2] == ta
    np.testing.assert_array_equal(_bits(one[-1][1][:ta + tl]), _bits(two[-1][1][:ta + tl]))      # one chunk of 3 = chunks of 2 and 1
    np.testing.assert_array_equal(_bits(U1), _bits(U2))
    assert info1["evaluations"] == NO * (T + 1) + 1 and info2["evaluations"] == NO * (T + 1) + 2
    # the parts through the pure entries
    Xd = torch.as_tensor(X0.reshape(K, H, da), device="cuda")
    al = auglag_state_new(Xd, 10.0, sc.m, lb=-1.0, ub=1.0)
    va = auglag_state_view(al, K, H, da, sc.m)
    inner = lbfgs_start(Xd, **lkw)                           # U = clip(X0)
    vi = lbfgs_state_view(inner, K, H, da, m)
    okw = dict(lb=-1.0, ub=1.0, history=m, gtol=1e-6, ftol=1e-12, inner_ticks=T)
    ev = lambda: G.rollout(pack, x0, vi["U"], cost, want_grad=True, want_traj=False, constraints=sc)      # noqa: E731
    for o in range(NO):
        start = Xd
        if o > 0:
            start = vi["X"].clone().view(K, H, da)
            vi["U"].copy_(start)
        r = ev()
        auglag_outer(al, r["cost"], r["g"], vi["U"], K, H, da, update=o > 0, conv=vi["converged"], **okw)
        M, dM = auglag_merit(r["cost"], r["grad"], r["g"], r["g_jac"], va["lam"], va["rho"])
        lbfgs_start(start, M, dM, state=inner, **lkw)
        for _ in range(T):
            r = ev()
            M, dM = auglag_merit(r["cost"], r["grad"], r["g"], r["g_jac"], va["lam"], va["rho"])
            lbfgs_tick(inner, M, dM, K, H, da, **lkw)
    vi["U"].copy_(vi["X"].view(K, H, da))
    r = ev()
    auglag_outer(al, r["cost"], r["g"], vi["U"], K, H, da, update=False, alive=vi["alive"], **okw)
    ws = one[-1][1]
    np.testing.assert_array_equal(_bits(al[:ta]), _bits(ws[:ta]))
    np.testing.assert_array_equal(_bits(inner[:tl]), _bits(ws[ta:ta + tl]))
    np.testing.assert_array_equal(_bits(U1), _bits(va["plan"]))
    assert c1 == float(al[3].item()) and info1["best"] == int(al[1].item())


@pytest.mark.parametrize("f", [0.1, 0.3])
def test_it_solves(G, f):
    """c1, K = 4 (row 0 the zero start), the defaults: 8 outer iterations x 25 ticks.  On the CPU (restatement on the oracle) row 0 ended at
    1.862348 / 1.874926, the other starts 5 - 7 % below.  Measured on an MI355X: f = 0.1: incumbents 1.862346 / 1.766236 / 1.839682 /
    1.736828, the best plan's reference cost 1.736828 (0.933 of the SLSQP figure) at max g = 3.5e-5; f = 0.3: 1.874938 / 1.799032 / 1.855027 /
    1.763889, reference cost 1.763889 (0.941) at max g = -4.8e-5; 8 outer iterations and 216 evaluations each."""
    from gaussian_process_mpc_amd.device_auglag import auglag_solve, auglag_state_fields
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_state_fields
    c = _problem(G)
    pb, gp, X0 = c["pb"], c["gp"], c["X0"]
    pack, cost, sc = _pack(G), _cost(G), _sc(G, f)
    H, da, x0, K, m = pb["H"], pb["da"], pb["x0"][0], 4, 8
    n = H * da
    g_free = reference_constraints(gp, H, x0, c["U_free"], c["A"], [c["b"][f]], [K95], want_jac=False)["g"].max()
    assert g_free > 0.05                                      # otherwise the test shows nothing
    log = []
    U, best_cost, info = auglag_solve(pack, x0, X0.reshape(K, H, da), cost, sc, lb=-1.0, ub=1.0, check_outer=1, callback=_log_into(log))
    print("f = %g: outer %d, evaluations %d, best %d, f %s, violation %s, rho %s, settled %s" % (f, info["outer"], info["evaluations"],
          info["best"], info["f"], info["violation"], info["rho"], info["settled"]))
    # the best plan by the CPU reference
    viol = reference_constraints(gp, H, x0, U, c["A"], [c["b"][f]], [K95], want_jac=False)["g"].max()
    ref_cost = reference_cost(gp, H, x0, U, pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], 1e-5)
    print("best plan: reference max g %.3e, reference cost %.6f (SLSQP single start: %.5f, ratio %.4f)" % (viol, ref_cost, SLSQP[f], ref_cost / SLSQP[f]))
    assert viol <= 1e-4 + 1e-6
    assert ref_cost <= SLSQP[f] * (1 + 1e-3)
    assert np.all(np.abs(U) <= 1.0) and np.all(np.abs(info["x"]) <= 1.0)
    assert info["feasible"][info["best"]] and best_cost == info["f"][info["best"]]
    np.testing.assert_array_equal(_bits(U.reshape(-1)), _bits(info["x"][info["best"]]))
    # every incumbent reported feasible is feasible by an independent device evaluation
    r = G.rollout(pack, x0, info["x"].reshape(K, H, da), cost, want_grad=False, want_traj=False, constraints=sc)
    gmax = r["g"].cpu().numpy().reshape(K, -1).max(axis=1)
    print("max g of the incumbents:", gmax)
    assert info["feasible"].any() and np.all(gmax[info["feasible"]] <= 1e-4)
    np.testing.assert_allclose(r["cost"].cpu().numpy(), info["f"], rtol=1e-12)
    # incumbent keys never increase; after every chunk the inner F is the merit at X with the state's multipliers and penalty
    prev = None
    for done, ws, off in log:
        s = auglag_state_fields(ws, K, H, da, sc.m)
        keys = list(zip(s["inc_v"], s["inc_f"]))
        if prev is not None:
            assert all(k2 <= k1 for k1, k2 in zip(prev, keys)), (done, prev, keys)
        prev = keys
        inner = lbfgs_state_fields(ws[off:], K, H, da, m)
        e = G.rollout(pack, x0, inner["X"].reshape(K, H, da), cost, want_grad=True, want_traj=False, constraints=sc)
        M, _ = AR.merit(e["cost"].cpu().numpy(), e["grad"].cpu().numpy().reshape(K, n), e["g"].cpu().numpy().reshape(K, -1),
                        e["g_jac"].cpu().numpy(), s["lam"], s["rho"])
        assert inner["alive"].all()
        np.testing.assert_allclose(inner["F"], M, rtol=1e-12)
    assert len(log) == info["outer"] <= 8


# ------------------------------------------------------------------------------------------------------------------------------
# 6. interface and edge cases
# ------------------------------------------------------------------------------------------------------------------------------
def test_mpc_interface_and_default_unchanged(G):
    from gaussian_process_mpc_amd.device_auglag import auglag_solve
    c = _problem(G)
    mpc, pb, X0 = c["mpc"], c["pb"], c["X0"]
    x0, H, da = pb["x0"][0], pb["H"], pb["da"]
    n = H * da
    assert mpc.solver is None and mpc.state_constraints is None
    before = c["U_free"]
    with pytest.raises(ValueError, match="lbfgs"):
        mpc.get_optimal_trajectory(x0, solver="auglag")      # no constraints set
    mpc.set_state_constraints(c["A"], [c["b"][0.3]], prob=0.95)
    with pytest.raises(NotImplementedError, match="state constraints"):
        mpc.get_optimal_trajectory(x0, solver="lbfgs")
    with pytest.raises(NotImplementedError, match="multi-start"):
        mpc.get_optimal_trajectory(x0, n_starts=4)
    saved = mpc.solver_used, mpc._solve_count
    mpc.solver_used, mpc._solve_count = None, 0              # (as a fresh object: no warm start, first seed)
    mpc.n_starts = 4
    mpc.auglag_options.update(outer=3, inner_ticks=10)
    plan = mpc.get_optimal_trajectory(x0, solver="auglag")
    info = mpc.last_solve_info
    assert plan.shape == (H, da) and mpc.solver_used == "device-auglag x4" and np.all(np.abs(plan) <= 1.0)
    assert {"f", "violation", "feasible", "x", "best", "rho", "lam", "outer", "evaluations", "settled", "alive", "success", "max_violation",
            "starts"} <= set(info)
    assert info["f"].shape == info["violation"].shape == info["rho"].shape == (4,) and info["x"].shape == (4, n)
    assert info["lam"].shape == (4, H) and info["starts"] == 4 and info["alive"].all() and info["outer"] <= 3
    assert info["success"] == bool(info["feasible"][info["best"]]) and info["max_violation"] == info["violation"][info["best"]]
    np.testing.assert_array_equal(mpc.last_traj, plan.reshape(-1))
    # the starts, the seed and the solve count are those of the unconstrained device search
    U, _, _ = auglag_solve(mpc.dynamics.pack(), x0, X0.reshape(4, H, da), mpc._cost_params(), mpc.state_constraints, lb=-1.0, ub=1.0,
                           **mpc.auglag_options)
    np.testing.assert_array_equal(_bits(U), _bits(plan))
    mpc.solver, mpc.n_starts = "auglag", 1                   # the attribute, one start, the warm start of a second solve
    plan1 = mpc.get_optimal_trajectory(x0)
    assert mpc.solver_used == "device-auglag x1" and plan1.shape == (H, da) and mpc.last_solve_info["f"].shape == (1,)
    mpc.full_covariance = True
    with pytest.raises(NotImplementedError, match="full-covariance"):
        mpc.get_optimal_trajectory(x0)
    mpc.full_covariance = False
    # the default solver is what it was
    mpc.clear_state_constraints()
    mpc.solver, mpc.n_starts = None, 1
    mpc.solver_used, mpc._solve_count = saved
    after = mpc.get_optimal_trajectory(x0)
    assert mpc.solver_used == c["used"]
    np.testing.assert_array_equal(_bits(after), _bits(before))


def test_nominal_pack(G):
    from gaussian_process_mpc_amd.device_auglag import auglag_solve
    c = _problem(G)
    pb, X0 = c["pb"], c["X0"]
    H, da, x0 = pb["H"], pb["da"], pb["x0"][1]
    cost = _cost(G)
    nom, plain = _pack(G, nominal=True), _pack(G)
    sc = G.StateConstraints([[1.0, 0.0]], [1.0], prob=0.95)
    kw = dict(lb=-1.0, ub=1.0, outer=3, inner_ticks=8, check_outer=0)
    Ua, ca, ia = auglag_solve(nom, x0, X0.reshape(4, H, da), cost, sc, **kw)
    Ub, cb, ib = auglag_solve(nom, x0, X0.reshape(4, H, da), cost, sc, **kw)
    np.testing.assert_array_equal(_bits(Ua), _bits(Ub))
    np.testing.assert_array_equal(_bits(ia["f"]), _bits(ib["f"]))
    assert ia["alive"].all() and np.isfinite(ia["f"]).all()
    r = G.rollout(nom, x0, ia["x"].reshape(4, H, da), cost, want_grad=False, want_traj=False, constraints=sc)
    gmax = r["g"].cpu().numpy().reshape(4, -1).max(axis=1)
    print("nominal pack: f %s, violation %s, max g %s" % (ia["f"], ia["violation"], gmax))
    assert np.all(gmax[ia["feasible"]] <= 1e-4)
    np.testing.assert_allclose(np.where(gmax <= 1e-4, 0.0, gmax), ia["violation"], rtol=1e-12)
    _, cp, _ = auglag_solve(plain, x0, X0.reshape(4, H, da), cost, sc, **kw)
    assert cp != ca                                          # (the model changes the problem)


def test_refusals_and_error_codes(G):
    from gaussian_process_mpc_amd import _lib
    from gaussian_process_mpc_amd.device_auglag import auglag_merit, auglag_outer, auglag_params, auglag_solve, auglag_state_new
    c = _problem(G)
    pb, X0 = c["pb"], c["X0"]
    H, da, x0 = pb["H"], pb["da"], pb["x0"][0]
    pack, cost, sc = _pack(G), _cost(G), _sc(G)
    X = X0.reshape(4, H, da)
    good = dict(lb=-1.0, ub=1.0, outer=1, inner_ticks=2, check_outer=0)
    for bad, text in ((dict(rho0=0.0), "rho0"), (dict(rho0=NAN), "rho0"), (dict(growth=-1.0), "growth"), (dict(growth=0.5), "growth"),
                      (dict(rho_max=0.0), "rho_max"), (dict(shrink=0.0), "shrink"), (dict(shrink=1.5), "shrink"), (dict(shrink=NAN), "shrink"),
                      (dict(feas_tol=-1e-9), "feas_tol"), (dict(lam_max=NAN), "lam_max"), (dict(inner_ticks=0), "inner_ticks"),
                      (dict(outer=-1), "n_outer"), (dict(history=0), "history"), (dict(gtol=-1.0), "gtol"), (dict(ftol=NAN), "ftol"),
                      (dict(lb=0.5, ub=0.25), r"lb\[0\]"), (dict(lb=[-1.0, NAN]), r"lb\[1\]")):
        with pytest.raises(G.GpmpcError, match="bad argument.*" + text):
            auglag_solve(pack, x0, X, cost, sc, **{**good, **bad})
    with pytest.raises(G.GpmpcError, match="bad argument.*n_starts"):
        auglag_solve(pack, x0, np.zeros((257, H, da)), cost, sc, **good)
    with pytest.raises(ValueError, match="state constraints"):
        auglag_solve(pack, x0, X, cost, None, **good)
    with pytest.raises(ValueError, match="check_outer"):
        auglag_solve(pack, x0, X, cost, sc, **{**good, "check_outer": -1})
    state = auglag_state_new(torch.as_tensor(X, device="cuda"), 10.0, 1)
    with pytest.raises(G.GpmpcError, match="bad argument.*shrink"):
        auglag_outer(state, np.zeros(4), np.zeros((4, H, 1)), X, 4, H, da, shrink=2.0)
    with pytest.raises(G.GpmpcError, match="workspace too small"):
        auglag_outer(state[:-32], np.zeros(4), np.zeros((4, H, 1)), X, 4, H, da)
    with pytest.raises(ValueError, match="shape"):
        auglag_merit(np.zeros(3), np.zeros((4, H, da)), np.zeros((4, H, 1)), np.zeros((4, H, H * da)), np.zeros((4, H)), np.ones(4))
    lib = G.lib()
    P = auglag_params(4, da, -1.0, 1.0, inner_ticks=2)
    nbytes = lib.gpmpc_auglag_solve_workspace_bytes(pack.handle, H, ctypes.byref(sc.c), ctypes.byref(P))
    assert nbytes > lib.gpmpc_auglag_state_bytes(4, H, da, 1) + lib.gpmpc_lbfgs_state_bytes(4, H, da, 8) > 0
    buf = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    ws = torch.zeros(nbytes // 8 + 32, dtype=torch.float64, device="cuda")
    call = lambda h, nb, first=0, no=1: lib.gpmpc_auglag_solve(h, H, _lib.ptr(buf[:2]), _lib.ptr(buf[64:64 + 4 * H * da]), ctypes.byref(cost.c),   # noqa: E731
                                                               ctypes.byref(sc.c), ctypes.byref(P), first, no, _lib.ptr(ws), nb, _lib.stream_ptr())
    assert call(pack.handle, nbytes - 1) == -4               # GPMPC_E_WORKSPACE
    assert call(pack.handle, nbytes, first=-1) == -1 and call(pack.handle, nbytes, no=-1) == -1
    h = ctypes.c_void_p()                                    # a pack that is not built: GPMPC_E_STATE
    assert lib.gpmpc_pack_create(ctypes.byref(h), 100, 2, 2) == 0
    try:
        assert call(h, nbytes) == -5
    finally:
        lib.gpmpc_pack_destroy(h)
    torch.cuda.synchronize()
    assert not ws.any()                                      # nothing was launched by any of the refused calls
    assert call(pack.handle, nbytes) == 0
    torch.cuda.synchronize()
    assert ws[4].item() == 4 and ws[5].item() == H * da and ws[6].item() == H
    assert call(pack.handle, nbytes, first=1, no=0) == 0     # a continuation that only refreshes the incumbents
    torch.cuda.synchronize()
    assert ws[4].item() == 4


def test_pendulum_closed_loop_three_steps(G):
    """The loop of tests/test_gpu_constraints.py::_pendulum_loop, three steps, |theta_dot| <= 0.6 at 95 % on every predicted state."""
    V = 0.6
    rng = np.random.default_rng(3)
    plant = G.PendulumPlant(init_state=(0.3, 0.0))
    S = np.stack((rng.uniform(-1, 1, 100), rng.uniform(-2, 2, 100)), axis=1)
    A = rng.uniform(-2, 2, (100, 1))
    nxt = np.array([G.PendulumPlant(init_state=s).step(a)[0] for s, a in zip(S, A)])
    mpc = G.RiskSensitiveMPC(-1.0, 5, 2, 1, np.diag([10.0, 0.1]), 0.01 * np.eye(1), nominal_models=G.LinearNominalModel.identity(2, 1))
    for g in mpc.dynamics.gpr_err:
        g.set_lambdas(np.array([1.0, 4.0, 4.0]))
        g.set_sigma_n(np.array(1e-2))
    mpc.dynamics.append_train_data(S, A, nxt)
    mpc.set_lb([-2.0])
    mpc.set_ub([2.0])
    mpc.set_state_bounds([None, -V], [None, V], 0.95)
    mpc.solver, mpc.n_starts = "auglag", 4
    log, solve = [], mpc.get_optimal_trajectory

    def logged(obs, **kw):
        plan = solve(obs, **kw)
        r = G.rollout(mpc.dynamics.pack(), obs, plan.reshape(1, 5, 1), mpc._cost_params(), want_grad=False, want_traj=False,
                      constraints=mpc.state_constraints)
        log.append((np.array(plan), mpc.solver_used, dict(mpc.last_solve_info), float(r["g"].max().item())))
        return plan
    mpc.get_optimal_trajectory = logged
    hist = G.Simulator(mpc, plant, num_iters=3, incremental=True).run()
    states = np.array([h[0] for h in hist])
    print("theta_dot visited %s, max g of the plans %s, outer iterations %s" % (states[:, 1], [g for _, _, _, g in log],
                                                                                 [i["outer"] for _, _, i, _ in log]))
    assert len(log) == 3 and all(s == "device-auglag x4" for _, s, _, _ in log)
    assert np.all(np.isfinite(states)) and all(np.all(np.abs(p) <= 2.0) and np.all(np.isfinite(p)) for p, _, _, _ in log)
    assert all(i["success"] and i["max_violation"] == 0.0 and i["alive"].all() for _, _, i, _ in log)
    assert all(g <= 1e-4 for _, _, _, g in log)              # the bound holds on every plan, by an independent evaluation
    assert np.all(np.abs(states[:, 1]) <= V)
