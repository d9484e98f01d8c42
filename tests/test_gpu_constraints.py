"""GPU tests of the state chance constraints: k_rollout_constraints (csrc/constraints.hip) through gpmpc_rollout_constraints and
gpmpc_rollout_constrained, against the float64 CPU reference of tests/constraints_reference.py (pinned oracle + autograd row by row, none
of the kernel's closed forms), and the constrained solve of RiskSensitiveMPC.

Tolerances follow from the project's own (means 1e-5, variances 1e-4 relative):
    |g - g_ref| <= 1e-5 sum_k |a_k mu_k| + 0.5e-4 kappa sd_ref + 1e-9        (d sd = d q / (2 sd): half the relative error of a variance)
and every Jacobian row and the whole matrix are held by the criterion the project uses for gradients (1e-4 relative, directional and in norm).
"""
import ctypes

import numpy as np
import pytest
import torch

from constraints_reference import reference_constraints, reference_cost
from nominal_reference import nominal_rollout, synth_nominal

pytestmark = pytest.mark.gpu

GRAD_RTOL = 1e-4
K95 = 1.6448536269514722
FORCE_TWO_LAUNCH = ("GPMPC_FUSED", "GPMPC_FUSED_SB", "GPMPC_PERSIST")

#        tag     config N    ds da H   gamma  shared
CASES = {"c1":  (1,     100, 2, 2, 10, 1e-5,  False),
         "c2":  (2,     200, 3, 1, 20, -1.0,  False),
         "c3":  (3,     449, 4, 1, 10, -1.0,  False),
         "c3s": (3,     449, 4, 1, 10, -1.0,  True),
         "d6":  (4,     300, 6, 2, 8,  -1.0,  False)}
BMAX = 64
_problems, _refs = {}, {}


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    return g


def _problem(tag):
    if tag not in _problems:
        from gaussian_process_mpc_amd.synth import synth_problem
        from oracle import gpmpc_oracle as O
        cfg, N, ds, da, H, gamma, shared = CASES[tag]
        pb = synth_problem(cfg, N, ds, da, H, BMAX, shared_lambda=shared)
        pb["gamma"] = gamma
        gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"])
        _problems[tag] = (pb, gp)
    return _problems[tag]


def _rows(ds):
    """Three mixed rows: an axis row at 95 %, a general row at kappa = 2, a general mean-only row (kappa = 0)."""
    rng = np.random.default_rng(77 + ds)
    A = rng.standard_normal((3, ds))
    A[0] = 0.0
    A[0, 0] = 1.0
    return A, np.array([0.5, 0.2, 0.1]), np.array([K95, 2.0, 0.0])


def _sc(G, ds):
    A, b, kap = _rows(ds)
    return G.StateConstraints(A, b, kappa=kap)


def _ref(tag, b, nominal):
    key = (tag, b, nominal)
    if key not in _refs:
        pb, gp = _problem(tag)
        A, bb, kap = _rows(pb["ds"])
        r = reference_constraints(gp, pb["H"], pb["x0"][b], pb["U"][b], A, bb, kap, nominal=synth_nominal(pb["ds"], pb["da"]) if nominal else None)
        assert np.all(np.isfinite(r["jac"])) and np.all(r["vars"] > 0)
        _refs[key] = r
    return _refs[key]


def _pack(G, tag, nominal=False):
    pb, gp = _problem(tag)
    return G.GPPack(pb["X"], pb["Y"], gp.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"], nominal=synth_nominal(pb["ds"], pb["da"]) if nominal else None)


def _cost(G, tag):
    pb = _problem(tag)[0]
    return G.CostParams(pb["gamma"], pb["Q"], pb["R"], x_ref=pb["x_ref"], u_ref=pb["u_ref"])


def _assert_grad(got, ref, what, quiet=False):
    """The project's gradient criterion (tests/test_gpu_nominal.py, restated): directional derivatives along the reference vector and three
    seeded directions, 1e-4 relative; and the whole vector in norm."""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    rng = np.random.default_rng(12345)
    dirs = [ref / np.linalg.norm(ref)] + [d / np.linalg.norm(d) for d in rng.standard_normal((3, ref.size))]
    for k, d in enumerate(dirs):
        a, e = float(got @ d), float(ref @ d)
        if not quiet:
            print("  %s: directional derivative %d: %.12g vs reference %.12g (rel %.2e)" % (what, k, a, e, abs(a - e) / abs(e)))
        assert abs(a - e) <= GRAD_RTOL * abs(e), (what, k, a, e)
    assert np.linalg.norm(got - ref) <= GRAD_RTOL * np.linalg.norm(ref), what


def _assert_g(got, ref, A, kap, what):
    """|g - g_ref| <= 1e-5 sum_k |a_k mu_k| + 0.5e-4 kappa sd_ref + 1e-9, element by element."""
    tol = 1e-5 * (np.abs(ref["means"][1:, None, :] * A[None, :, :])).sum(axis=2) + 0.5e-4 * kap[None, :] * ref["sd"] + 1e-9
    err = np.abs(got - ref["g"])
    print("  %s: max |g - g_ref| %.3e, smallest bound %.3e, largest ratio %.3e" % (what, err.max(), tol.min(), (err / tol).max()))
    assert np.all(err <= tol), (what, err.max())


def _assert_jac(got, ref, H, m_c, da, what):
    worst = 0.0
    for i in range(H * m_c):
        _assert_grad(got[i], ref[i], "%s row %d" % (what, i), quiet=True)
        worst = max(worst, np.linalg.norm(got[i] - ref[i]) / np.linalg.norm(ref[i]))
    print("  %s: worst row, relative error in norm %.3e" % (what, worst))
    _assert_grad(got, ref, what + " whole matrix")
    for t in range(1, H + 1):                                # causality: exact zeros, sign included
        blk = got[(t - 1) * m_c:t * m_c, t * da:]
        assert not np.any(blk) and not np.any(np.signbit(blk)), (what, t)


def _rollout_jac(pack, x0, U):
    from gaussian_process_mpc_amd._lib import lib, check, ptr, stream_ptr
    dev = pack.device
    x0 = torch.as_tensor(np.ascontiguousarray(x0), device=dev)
    U = torch.as_tensor(np.ascontiguousarray(U), device=dev)
    B, H, da = U.shape
    ds = pack.ds
    e = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    means, vars_, jac = e(B, H + 1, ds), e(B, H + 1, ds), e(B, H, 2 * ds, 2 * ds + da)
    ws = pack.workspace(lib().gpmpc_rollout_jac_workspace_bytes(pack.handle, B, H))
    check(lib().gpmpc_rollout_jac(pack.handle, B, H, ptr(x0), ptr(U), ptr(means), ptr(vars_), ptr(jac), ctypes.c_void_p(ws.data_ptr()),
                                  ws.numel(), stream_ptr()), "gpmpc_rollout_jac")
    torch.cuda.synchronize()
    return means, vars_, jac


def _pure(sc, means, vars_, jac, ds, da, fill=float("nan")):
    """gpmpc_rollout_constraints into buffers pre-filled with NaN: a store the kernel misses shows."""
    from gaussian_process_mpc_amd._lib import lib, check, ptr, stream_ptr
    B, H1, _ = means.shape
    H = H1 - 1
    g = torch.full((B, H, sc.m), fill, dtype=torch.float64, device=means.device)
    gj = torch.full((B, H * sc.m, H * da), fill, dtype=torch.float64, device=means.device) if jac is not None else None
    check(lib().gpmpc_rollout_constraints(B, H, ds, da, ctypes.byref(sc.c), ptr(means), ptr(vars_), ptr(jac), ptr(g), ptr(gj), stream_ptr()),
          "gpmpc_rollout_constraints")
    torch.cuda.synchronize()
    return g, gj


# ------------------------------------------------------------------------------------------------------------------------------
# 1. against the reference: default plan, forced two-launch plan, nominal pack
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "two_launch", "nominal"])
@pytest.mark.parametrize("tag", ["c1", "c2", "c3", "c3s", "d6"])
def test_against_the_reference(G, tag, mode, monkeypatch):
    pb, gp = _problem(tag)
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    A, bb, kap = _rows(ds)
    sc, cost = _sc(G, ds), _cost(G, tag)
    if mode == "two_launch":
        for k in FORCE_TWO_LAUNCH:
            monkeypatch.setenv(k, "0")
    pack = _pack(G, tag, nominal=mode == "nominal")           # (overrides are read at pack creation)
    if mode == "two_launch":
        for k in FORCE_TWO_LAUNCH:
            monkeypatch.delenv(k)
    B = 2
    plan = pack.plan(B, H, want_grad=True)
    print("%s %s: %s" % (tag, mode, plan))
    if mode == "default":
        assert plan["launches_per_step"] in (0, 1) and (plan["form"].startswith("fused") or plan["form"] == "persist"), plan
    else:
        assert plan["launches_per_step"] == 2 and plan["form"].startswith("head+pair"), plan
        assert (plan.get("nominal") == 1) == (mode == "nominal")
    r = G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=True, constraints=sc)
    v = G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=False, constraints=sc)          # the kernel's value-only path
    torch.cuda.synchronize()
    assert tuple(r["g"].shape) == (B, H, 3) and tuple(r["g_jac"].shape) == (B, H * 3, H * da) and "g_jac" not in v and "grad" not in v
    np.testing.assert_array_equal(v["g"].cpu().numpy(), r["g"].cpu().numpy())
    for b in range(B):
        ref = _ref(tag, b, mode == "nominal")
        what = "%s %s [%d] %s" % (tag, mode, b, plan["form"])
        np.testing.assert_allclose(r["means"][b].cpu().numpy(), ref["means"], rtol=1e-5, atol=1e-9)
        np.testing.assert_allclose(r["vars"][b].cpu().numpy(), ref["vars"], rtol=1e-4, atol=1e-12)
        _assert_g(r["g"][b].cpu().numpy(), ref, A, kap, what)
        _assert_jac(r["g_jac"][b].cpu().numpy(), ref["jac"], H, 3, da, what)
    if mode == "nominal":                                    # ... and against nominal_reference.nominal_rollout's own trajectory
        W, c = synth_nominal(ds, da)
        nr = nominal_rollout(gp, W, c, H, pb["x0"][0], pb["U"][0], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], pb["gamma"], want_grad=False)
        sd = np.sqrt(nr["vars"][1:] @ (A * A).T)
        g_nr = nr["means"][1:] @ A.T + kap[None, :] * sd - bb[None, :]
        _assert_g(r["g"][0].cpu().numpy(), {"g": g_nr, "means": nr["means"], "sd": sd}, A, kap, "%s nominal_rollout trajectory" % tag)
        from oracle import gpmpc_oracle as O                 # none of this could pass on a rollout that ignores the model
        plain = O.objective_and_gradient(gp, H, pb["x0"][0], pb["U"][0], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], pb["gamma"], mode="o2", want_grad=False)
        assert np.max(np.abs(plain["means"][1:] - nr["means"][1:])) > 1e-3


# ------------------------------------------------------------------------------------------------------------------------------
# 2. causality on a wide problem: several waves per trajectory, every element stored
# ------------------------------------------------------------------------------------------------------------------------------
def test_causality_and_complete_stores_over_several_waves(G):
    """H da = 160 columns = three waves per trajectory (the last one partly filled); m_c = 16 rows (the maximum); NaN-filled outputs."""
    rng = np.random.default_rng(5)
    B, H, ds, da, m_c = 3, 80, 3, 2, 16
    dev = G.require_gpu()
    means = torch.as_tensor(rng.standard_normal((B, H + 1, ds)), device=dev)
    vars_ = torch.as_tensor(rng.uniform(0.01, 0.1, (B, H + 1, ds)), device=dev)
    jac = torch.as_tensor(0.5 * rng.standard_normal((B, H, 2 * ds, 2 * ds + da)), device=dev)
    sc = G.StateConstraints(rng.standard_normal((m_c, ds)), rng.standard_normal(m_c), kappa=rng.uniform(0, 2, m_c))
    g, gj = _pure(sc, means, vars_, jac, ds, da)
    g, gj = g.cpu().numpy(), gj.cpu().numpy()
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(gj))                 # nothing left of the NaN fill
    for t in range(1, H + 1):
        blk = gj[:, (t - 1) * m_c:t * m_c, t * da:]
        assert not np.any(blk) and not np.any(np.signbit(blk)), t
        assert np.all(gj[:, (t - 1) * m_c:t * m_c, (t - 1) * da:t * da] != 0.0)
    # the sweep itself, in numpy (hand-made inputs: this is the recursion of DESIGN.md section 3b, not the reference)
    Jn, Vn, An, Kn = jac.cpu().numpy(), vars_.cpu().numpy(), sc.A, sc.kappa
    for b in range(B):
        S = np.zeros((2 * ds, H * da))
        for t in range(1, H + 1):
            S = Jn[b, t - 1][:, :2 * ds] @ S
            S[:, (t - 1) * da:t * da] = Jn[b, t - 1][:, 2 * ds:]
            sd = np.sqrt((An * An) @ Vn[b, t])
            rows = An @ S[:ds] + (Kn / (2 * sd))[:, None] * ((An * An) @ S[ds:])
            np.testing.assert_allclose(gj[b, (t - 1) * m_c:t * m_c], rows, rtol=1e-10, atol=1e-10 * np.abs(rows).max())


# ------------------------------------------------------------------------------------------------------------------------------
# 3. consistency with the existing backward pass
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["c1", "c3", "d6"])
def test_jacobian_transpose_times_weights_equals_rollout_vjp(G, tag):
    from gaussian_process_mpc_amd._lib import lib, check, ptr, stream_ptr
    pb, _ = _problem(tag)
    ds, da, H, B = pb["ds"], pb["da"], pb["H"], 4
    A, bb, kap = _rows(ds)
    sc, pack = _sc(G, ds), _pack(G, tag)
    means, vars_, jac = _rollout_jac(pack, pb["x0"][:B], pb["U"][:B])
    g, gj = _pure(sc, means, vars_, jac, ds, da)
    w = np.random.default_rng(9).standard_normal((B, H, 3))
    sd = np.sqrt(vars_.cpu().numpy()[:, 1:] @ (A * A).T)                                       # (B, H, m_c)
    gm, gv = np.zeros((B, H + 1, ds)), np.zeros((B, H + 1, ds))
    gm[:, 1:] = w @ A
    gv[:, 1:] = (w * kap[None, None, :] / (2 * sd)) @ (A * A)
    gm_d, gv_d = torch.as_tensor(gm, device=pack.device), torch.as_tensor(gv, device=pack.device)
    gU = torch.empty((B, H, da), dtype=torch.float64, device=pack.device)
    check(lib().gpmpc_rollout_vjp(B, H, ds, da, ptr(jac), ptr(gm_d), ptr(gv_d), ptr(gU), None, stream_ptr()), "gpmpc_rollout_vjp")
    torch.cuda.synchronize()
    mine = np.einsum("brc,br->bc", gj.cpu().numpy(), w.reshape(B, H * 3))
    theirs = gU.cpu().numpy().reshape(B, H * da)
    scale = np.abs(theirs).max()
    print("  %s: max |J^T w - vjp| %.3e at scale %.3e" % (tag, np.abs(mine - theirs).max(), scale))
    np.testing.assert_allclose(mine, theirs, rtol=1e-12, atol=1e-12 * scale)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. batch independence, 5. one pass equals two
# ------------------------------------------------------------------------------------------------------------------------------
def test_batch_of_64_equals_64_single_calls_bit_for_bit(G):
    pb, _ = _problem("c1")
    ds, da = pb["ds"], pb["da"]
    sc, pack = _sc(G, ds), _pack(G, "c1")
    means, vars_, jac = _rollout_jac(pack, pb["x0"], pb["U"])
    g, gj = _pure(sc, means, vars_, jac, ds, da)
    gv, _ = _pure(sc, means, vars_, None, ds, da)
    np.testing.assert_array_equal(gv.cpu().numpy(), g.cpu().numpy())
    for b in range(BMAX):
        g1, gj1 = _pure(sc, means[b:b + 1].contiguous(), vars_[b:b + 1].contiguous(), jac[b:b + 1].contiguous(), ds, da)
        np.testing.assert_array_equal(g1[0].cpu().numpy(), g[b].cpu().numpy())
        np.testing.assert_array_equal(gj1[0].cpu().numpy(), gj[b].cpu().numpy())


@pytest.mark.parametrize("tag,B", [("c1", 1), ("c2", 1), ("c3", 1), ("c3", BMAX), ("c3s", 16), ("d6", 2)])
def test_one_pass_equals_rollout_then_jacobians_then_constraints(G, tag, B):
    pb, _ = _problem(tag)
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    sc, pack, cost = _sc(G, ds), _pack(G, tag), _cost(G, tag)
    one = G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=True, constraints=sc)
    two = G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=True)
    torch.cuda.synchronize()
    print("%s B=%d: %s" % (tag, B, pack.plan(B, H)))
    for key in ("cost", "grad", "means", "vars"):
        np.testing.assert_array_equal(one[key].cpu().numpy(), two[key].cpu().numpy(), err_msg=key)
    means, vars_, jac = _rollout_jac(pack, pb["x0"][:B], pb["U"][:B])
    g, gj = _pure(sc, means, vars_, jac, ds, da)
    np.testing.assert_array_equal(one["g"].cpu().numpy(), g.cpu().numpy())
    np.testing.assert_array_equal(one["g_jac"].cpu().numpy(), gj.cpu().numpy())
    # the wrapper of the pure entry
    w = G.rollout_constraints(means, vars_, jac, sc, ds, da)
    np.testing.assert_array_equal(w["g_jac"].cpu().numpy(), gj.cpu().numpy())
    np.testing.assert_array_equal(G.rollout_constraints(means, vars_, None, sc, ds, da)["g"].cpu().numpy(), g.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------------------
# 6. edge semantics on hand-made inputs
# ------------------------------------------------------------------------------------------------------------------------------
def test_non_positive_and_nan_variances(G):
    rng = np.random.default_rng(11)
    B, H, ds, da = 1, 4, 2, 1
    dev = G.require_gpu()
    means = rng.standard_normal((B, H + 1, ds))
    vars_ = rng.uniform(0.01, 0.1, (B, H + 1, ds))
    jac = 0.5 * rng.standard_normal((B, H, 2 * ds, 2 * ds + da))
    A = np.array([[1.0, 0.0], [0.5, 2.0]])
    bb, kap = np.array([0.3, -0.2]), np.array([K95, 1.0])
    sc = G.StateConstraints(A, bb, kappa=kap)
    vars_[0, 2, 0] = -0.02          # step 2: row 0 has q = -0.02 < 0; row 1 has q = 0.25 (-0.02) + 4 var_1 > 0
    vars_[0, 3, :] = [0.0, 0.05]    # step 3: row 0 has q = 0 exactly
    t_ = lambda a: torch.as_tensor(a, device=dev)  # noqa: E731
    g, gj = _pure(sc, t_(means), t_(vars_), t_(jac), ds, da)
    g, gj = g.cpu().numpy()[0], gj.cpu().numpy()[0]
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(gj))
    S = np.zeros((2 * ds, H * da))
    for t in range(1, H + 1):
        S = jac[0, t - 1][:, :2 * ds] @ S
        S[:, (t - 1) * da:t * da] = jac[0, t - 1][:, 2 * ds:]
        q = (A * A) @ vars_[0, t]
        for r in range(2):
            mean_part = A[r] @ S[:ds]
            if q[r] <= 0:                                    # sd = 0: the row is its mean part, in value and derivative
                assert t in (2, 3) and r == 0
                np.testing.assert_allclose(g[t - 1, r], A[r] @ means[0, t] - bb[r], rtol=1e-14, atol=1e-15)
                np.testing.assert_allclose(gj[(t - 1) * 2 + r], mean_part, rtol=1e-13, atol=1e-15)
            else:
                sd = np.sqrt(q[r])
                np.testing.assert_allclose(g[t - 1, r], A[r] @ means[0, t] + kap[r] * sd - bb[r], rtol=1e-14, atol=1e-15)
                np.testing.assert_allclose(gj[(t - 1) * 2 + r], mean_part + kap[r] / (2 * sd) * ((A[r] * A[r]) @ S[ds:]), rtol=1e-12, atol=1e-14)
    # a NaN variance at step 3: the rows of step 3 are NaN (values and derivatives, causal zeros kept), no other step's
    vars_[0, 3, :] = [float("nan"), 0.05]
    g2, gj2 = _pure(sc, t_(means), t_(vars_), t_(jac), ds, da)
    g2, gj2 = g2.cpu().numpy()[0], gj2.cpu().numpy()[0]
    assert np.all(np.isnan(g2[2])) and np.all(np.isnan(gj2[4:6, :3 * da])) and not np.any(gj2[4:6, 3 * da:])
    keep = [0, 1, 3]
    np.testing.assert_array_equal(g2[keep], g[keep])
    rows = [i for i in range(H * 2) if i not in (4, 5)]
    np.testing.assert_array_equal(gj2[rows], gj[rows])


# ------------------------------------------------------------------------------------------------------------------------------
# 7. solve
# ------------------------------------------------------------------------------------------------------------------------------
def _mpc_c1(G):
    from oracle import gpmpc_oracle as O
    pb = _problem("c1")[0]
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    mpc = G.RiskSensitiveMPC(pb["gamma"], H, ds, da, pb["Q"], pb["R"])
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


@pytest.mark.parametrize("f,cpu_cost", [(0.1, 1.86235), (0.3, 1.87492)])
def test_constrained_solve(G, f, cpu_cost):
    """synth_problem(1, 100, 2, 2, 10, .) trajectory 0, gamma = 1e-5, inputs within +-1, start U = 0.  One row on state 0 at 95 %,
    b = top - f span of mu_t0 + kappa sd_t0 (t = 1..H) along the unconstrained optimum.  CPU figures of the same construction with the
    reference alone (SLSQP, ftol 1e-10): unconstrained cost 1.86054; f = 0.1: violated by 0.068, cost 1.86235; f = 0.3: by 0.205, 1.87492."""
    mpc, gp, pb = _mpc_c1(G)
    H, x0 = pb["H"], pb["x0"][0]
    rc = lambda U: reference_cost(gp, H, x0, U, pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], pb["gamma"])  # noqa: E731
    U_free = mpc.get_optimal_trajectory(x0)
    assert mpc.solver_used == "scipy-lbfgsb" or mpc.solver_used == "ipopt"
    cost_free = rc(U_free)
    print("unconstrained: reference cost %.6f (CPU solve: 1.86054)" % cost_free)
    np.testing.assert_allclose(cost_free, 1.86054, rtol=1e-3)
    A = np.array([[1.0, 0.0]])
    along = reference_constraints(gp, H, x0, U_free, A, [0.0], [K95], want_jac=False)["g"][:, 0]        # mu_t0 + kappa sd_t0
    top, span = along.max(), along.max() - along.min()
    b = top - f * span
    g_free = reference_constraints(gp, H, x0, U_free, A, [b], [K95], want_jac=False)["g"]
    print("f = %g: b = %.6f, the unconstrained plan violates the row by %.4f" % (f, b, g_free.max()))
    assert g_free.max() > 0.05                                # otherwise the test shows nothing
    mpc.set_state_constraints(A, [b], prob=0.95)
    U_con = mpc.get_optimal_trajectory(x0)
    info = mpc.last_solve_info
    print("constrained: %s %s" % (mpc.solver_used, info))
    if mpc.solver_used == "scipy-slsqp":
        assert info["success"], info
    ref = reference_constraints(gp, H, x0, U_con, A, [b], [K95], want_jac=False)
    cost_con = rc(U_con)
    print("constrained: reference max g %.3e, reference cost %.6f (CPU solve: %.5f, rel %.2e)"
          % (ref["g"].max(), cost_con, cpu_cost, abs(cost_con - cpu_cost) / cpu_cost))
    assert ref["g"].max() <= 1e-6
    assert np.all(np.abs(U_con) <= 1.0 + 1e-9)
    assert cost_con >= cost_free - 1e-9
    np.testing.assert_allclose(cost_con, cpu_cost, rtol=1e-3)


# ------------------------------------------------------------------------------------------------------------------------------
# 8. closed loop
# ------------------------------------------------------------------------------------------------------------------------------
def _pendulum_loop(G, V, steps=24):
    """Pendulum from theta = 0.3 towards upright, identity nominal model, 100 pre-training transitions, H = 5, Q = diag(10, 0.1): the
    unconstrained controller swings back at up to ~0.87 rad/s (predicted kappa sd of theta_dot: 0.07 ... 0.13 over the horizon)."""
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
    if V is not None:
        mpc.set_state_bounds([None, -V], [None, V], 0.95)
    log, solve = [], mpc.get_optimal_trajectory

    def logged(obs, **kw):
        plan = solve(obs, **kw)
        log.append((mpc.solver_used, None if mpc.last_solve_info is None else dict(mpc.last_solve_info)))
        return plan
    mpc.get_optimal_trajectory = logged
    hist = G.Simulator(mpc, plant, num_iters=steps, incremental=True).run()
    return np.array([h[0][1] for h in hist]), log


def test_closed_loop_with_a_chance_bound_on_theta_dot(G):
    """|theta_dot| <= 0.6 at 95 % on every predicted state.  The bound is fixed from the same loop on the CPU reference (SLSQP on the oracle
    with the identity nominal model): without it the loop reaches 0.868 rad/s, with it 0.535, every solve succeeds and the bound is
    active (max g ~ 1e-10) for ten steps."""
    V = 0.6
    free, _ = _pendulum_loop(G, None)
    print("without the bound: largest |theta_dot| visited %.4f" % np.abs(free).max())
    assert np.abs(free).max() > V                             # otherwise the test shows nothing
    speed, log = _pendulum_loop(G, V)
    print("with |theta_dot| <= %.2f: largest visited %.4f" % (V, np.abs(speed).max()))
    print("  max predicted g per step:", np.array2string(np.array([i["max_violation"] for _, i in log if i]), precision=2, max_line_width=200))
    assert len(log) == 24
    for k, (solver, info) in enumerate(log):
        if solver == "ipopt":
            continue
        assert solver == "scipy-slsqp" and info["success"], (k, solver, info)
        assert info["max_violation"] <= 1e-6, (k, info)
    assert min(i["max_violation"] for _, i in log if i) < -1e-3 < max(i["max_violation"] for _, i in log if i)      # active at some steps, slack at others


# ------------------------------------------------------------------------------------------------------------------------------
# 9. refusals, and clearing
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_clearing(G):
    mpc, gp, pb = _mpc_c1(G)
    H, da, x0 = pb["H"], pb["da"], pb["x0"][0]
    pack, cost, sc = mpc.dynamics.pack(), mpc._cost_params(), _sc(G, pb["ds"])
    with pytest.raises(ValueError, match="graph"):
        G.rollout(pack, x0, pb["U"][0], cost, graph=True, constraints=sc)
    with pytest.raises(ValueError, match="precision"):
        G.rollout(pack, x0, pb["U"][0], cost, want_grad=False, precision="fp32acc", constraints=sc)
    with pytest.raises(ValueError, match="state coefficients"):
        G.rollout(pack, x0, pb["U"][0], cost, constraints=G.StateConstraints(np.ones((1, 3)), 1.0, kappa=0.0))
    mpc.set_state_constraints([1.0, 0.0], 5.0, prob=0.95)
    with pytest.raises(NotImplementedError, match="multi-start"):
        mpc.get_optimal_trajectory(x0, n_starts=4)
    mpc.full_covariance = True
    with pytest.raises(NotImplementedError, match="full-covariance"):
        mpc.get_optimal_trajectory(x0)
    with pytest.raises(NotImplementedError, match="full-covariance"):
        mpc.evaluate_batch(pb["U"][:2], x0, constraints=True)
    mpc.curr_state = torch.tensor(x0, dtype=torch.float64, device=mpc.device)
    with pytest.raises(NotImplementedError, match="full-covariance"):
        mpc.constraints(np.zeros(H * da))
    mpc.full_covariance = False
    # the callbacks on one x: one evaluation, consistent with the batched screen
    x = pb["U"][0].reshape(-1).copy()
    g, jac = mpc.constraints(x), mpc.jacobian(x)
    assert g.shape == (H,) and jac.shape == (H * H * da,) and mpc.objective(x) == mpc.curr_cost
    scr = mpc.evaluate_batch(pb["U"][:3], x0, constraints=True)
    assert tuple(scr["g"].shape) == (3, H, 1) and tuple(scr["g_jac"].shape) == (3, H, H * da)
    np.testing.assert_array_equal(scr["g"][0].cpu().numpy().reshape(-1), g)
    np.testing.assert_array_equal(scr["g_jac"][0].cpu().numpy().reshape(-1), jac)
    assert "g_jac" not in mpc.evaluate_batch(pb["U"][:3], x0, want_grad=False, constraints=True)
    # a loose row (b = 5): the constrained solve succeeds with the constraint inactive
    mpc.get_optimal_trajectory(x0)
    if mpc.solver_used != "ipopt":
        assert mpc.solver_used == "scipy-slsqp" and mpc.last_solve_info["success"] and mpc.last_solve_info["max_violation"] < 0
    # clearing restores today's path
    mpc.clear_state_constraints()
    assert mpc.constraints(x) == 0 and not np.any(mpc.jacobian(x)) and mpc.jacobian(x).shape == x.shape
    with pytest.raises(ValueError):
        mpc.evaluate_batch(pb["U"][:3], x0, constraints=True)
    mpc.get_optimal_trajectory(x0)
    if mpc.solver_used != "ipopt":
        assert mpc.solver_used == "scipy-lbfgsb"
    # the C entry on a pack that is not built, and with flags it does not take
    from gaussian_process_mpc_amd import _lib
    from gaussian_process_mpc_amd._lib import lib
    h = ctypes.c_void_p()
    assert lib().gpmpc_pack_create(ctypes.byref(h), 10, 2, 1) == 0
    try:
        fake = ctypes.c_void_p(4096)
        call = lambda flags: lib().gpmpc_rollout_constrained(h, 1, 4, fake, fake, ctypes.byref(cost.c), ctypes.byref(sc.c), flags, None,  # noqa: E731
                                                             None, fake, fake, fake, fake, fake, 1 << 20, None)
        assert call(_lib.WANT_GRAD) == -5
        assert call(_lib.WANT_GRAD | _lib.USE_GRAPH) == -1 and b"GPMPC_WANT_GRAD" in lib().gpmpc_last_error()
    finally:
        lib().gpmpc_pack_destroy(h)
