"""GPU tests of the full-covariance rollout under chance constraints and the device solvers: k_fc_pack_jac (csrc/fullcov_cons.hip) through
gpmpc_rollout_fullcov_jac and gpmpc_rollout_fullcov_constrained, the *_solve_fullcov entries, and propagation = "moment_matching_full" of
RiskSensitiveMPC -- against the float64 CPU reference of tests/fullcov_cons_reference.py (pinned oracle + autograd row by row, none of the
kernels' closed forms).  Cases and rows are those of tests/test_gpu_constraints.py.

Tolerances: |g - g_ref| <= 1e-5 sum_k |a_k mu_k| + kappa dq / (2 sd_ref) + 1e-9 with dq = sum_kl |a_k a_l| (1e-4 |Sigma_kl| + 1e-6 max |Sigma_t|)
(``fullcov_cons_reference.g_tolerance``: the project's covariance tolerance pushed through the definition); every Jacobian row and the whole
matrix by the project's gradient criterion (1e-4 directional and in norm); causality zeros exact, sign included.
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import fullcov_cons_reference as F
import noise_reference as NR
import test_gpu_constraints as TC

pytestmark = pytest.mark.gpu

TAGS = ("c1", "c2", "c3", "c3s", "d6")
FORMS = {"two_launch": "1", "four_launch": "0"}
_refs, _packs = {}, {}


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    return g


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@contextlib.contextmanager
def _tuning(pack, env):
    """GPMPC_* overrides for the calls inside; restored, and the pack's tuning re-read, whatever happens."""
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        pack.reload_tuning()
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        pack.reload_tuning()


def _ref(tag, b):
    """The reference of plan b of a case, with its Jacobian: computed once, shared, never written."""
    if (tag, b) not in _refs:
        pb, gp = TC._problem(tag)
        A, bb, kap = TC._rows(pb["ds"])
        r = F.reference_fullcov_constraints(gp, pb["H"], pb["x0"][b], pb["U"][b], A, bb, kap)
        assert np.all(np.isfinite(r["jac"])) and r["q"].min() > 0
        _refs[(tag, b)] = r
    return _refs[(tag, b)]


def _pack(G, tag):
    if tag not in _packs:
        pb, gp = TC._problem(tag)
        _packs[tag] = G.GPPack(pb["X"], pb["Y"], gp.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"], fullcov=True)
    return _packs[tag]


def _assert_g(got, ref, A, kap, what):
    tol = F.g_tolerance(ref, A, kap)
    err = np.abs(got - ref["g"])
    print("  %s: max |g - g_ref| %.3e, smallest bound %.3e, largest ratio %.3e" % (what, err.max(), tol.min(), (err / tol).max()))
    assert np.all(err <= tol), (what, err.max())


# ------------------------------------------------------------------------------------------------------------------------------
# 1. against the reference, both forms of the rollout
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("tag", TAGS)
def test_against_the_reference(G, tag, form):
    pb, _ = TC._problem(tag)
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    A, bb, kap = TC._rows(ds)
    sc, cost, pack = TC._sc(G, ds), TC._cost(G, tag), _pack(G, tag)
    B = 2
    with _tuning(pack, {"GPMPC_FC_FORM": FORMS[form]}):
        plan = pack.plan_fullcov(B, H)
        print("%s %s: %s" % (tag, form, plan))
        assert plan["form"] == form, plan
        if tag == "c3s":
            assert pack.shared_lambda and (form == "four_launch" or "shared_cross_units" in plan)
        r = G.rollout_fullcov(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=True, constraints=sc)
        v = G.rollout_fullcov(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=False, constraints=sc)
        torch.cuda.synchronize()
    assert tuple(r["g"].shape) == (B, H, 3) and tuple(r["g_jac"].shape) == (B, H * 3, H * da) and "g_jac" not in v and "grad" not in v
    assert _same(v["g"], r["g"])
    for b in range(B):
        ref = _ref(tag, b)
        what = "%s %s [%d]" % (tag, form, b)
        np.testing.assert_allclose(r["means"][b].cpu().numpy(), ref["means"], rtol=1e-5, atol=1e-9)
        np.testing.assert_allclose(r["covs"][b].cpu().numpy(), ref["covs"], rtol=1e-4, atol=1e-6 * np.abs(ref["covs"]).max())
        _assert_g(r["g"][b].cpu().numpy(), ref, A, kap, what)
        TC._assert_jac(r["g_jac"][b].cpu().numpy(), ref["jac"], H, 3, da, what)
        # the diagonal rule would not pass here (tests/test_host_fullcov_cons.py holds the factor)
        assert (np.abs(ref["g_diag"] - ref["g"]) / F.g_tolerance(ref, A, kap))[:, 1].max() >= 50.0


# ------------------------------------------------------------------------------------------------------------------------------
# 2. bit for bit
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_bit_for_bit(G, tag):
    from gaussian_process_mpc_amd.linearised import linearised_fc_constraints
    pb, _ = TC._problem(tag)
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    sc, cost, pack = TC._sc(G, ds), TC._cost(G, tag), _pack(G, tag)
    B = 3
    x0, U = pb["x0"][:B], pb["U"][:B]
    r = G.rollout_fullcov(pack, x0, U, cost, want_grad=True, constraints=sc)
    plain = G.rollout_fullcov(pack, x0, U, cost, want_grad=True)
    for k in ("cost", "grad", "means", "covs"):
        assert _same(r[k], plain[k]), k
    v = G.rollout_fullcov(pack, x0, U, cost, want_grad=False, constraints=sc)
    plain_v = G.rollout_fullcov(pack, x0, U, cost, want_grad=False)
    for k in ("cost", "means", "covs"):
        assert _same(v[k], plain_v[k]), k
    assert _same(v["g"], r["g"])
    j = G.rollout_fullcov_jac(pack, x0, U)
    p = ds + ds * (ds + 1) // 2
    assert tuple(j["jac"].shape) == (B, H, p, p + da) and bool(torch.isfinite(j["jac"]).all())
    assert _same(j["means"], r["means"]) and _same(j["covs"], r["covs"])
    pure = linearised_fc_constraints(j["means"], j["covs"], j["jac"], sc, ds, da)
    assert _same(pure["g"], r["g"]) and _same(pure["g_jac"], r["g_jac"])
    again = G.rollout_fullcov(pack, x0, U, cost, want_grad=True, constraints=sc)
    for k in ("cost", "grad", "means", "covs", "g", "g_jac"):
        assert _same(again[k], r[k]), k
    assert _same(G.rollout_fullcov_jac(pack, x0, U)["jac"], j["jac"])
    # a batch is its trajectories
    one = G.rollout_fullcov(pack, x0[1:2], U[1:2], cost, want_grad=True, constraints=sc)
    if pack.plan_fullcov(1, H)["form"] == pack.plan_fullcov(B, H)["form"]:
        TC._assert_grad(one["g_jac"][0].cpu().numpy(), r["g_jac"][1].cpu().numpy(), "%s B = 1 against row 1 of B = 3" % tag, quiet=True)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the packing against the adjoint sweep of the rollout itself
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("tag", TAGS)
def test_packing_against_the_adjoint(G, tag, form):
    """gpmpc_linearised_fc_vjp over the packed Jacobians, seeded by gpmpc_cost_grad on the returned trajectory, plus the input-cost gradient,
    against the gradient of gpmpc_rollout_fullcov (k_fc_tail's sweep over the UNPACKED Jacobians): two independent sweeps over the same
    numbers."""
    from gaussian_process_mpc_amd._lib import check, lib, ptr, stream_ptr
    from gaussian_process_mpc_amd.linearised import linearised_fc_vjp
    pb, _ = TC._problem(tag)
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    cost, pack = TC._cost(G, tag), _pack(G, tag)
    B = 2
    with _tuning(pack, {"GPMPC_FC_FORM": FORMS[form]}):
        assert pack.plan_fullcov(B, H)["form"] == form
        r = G.rollout_fullcov(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=True)
        j = G.rollout_fullcov_jac(pack, pb["x0"][:B], pb["U"][:B])
    dev = pack.device
    U = torch.as_tensor(np.ascontiguousarray(pb["U"][:B]), device=dev)
    e = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=dev)  # noqa: E731
    c, dm, dS, dU = e(B), e(B, H + 1, ds), e(B, H + 1, ds, ds), e(B, H, da)
    check(lib().gpmpc_cost_grad(B, H, ds, da, ctypes.byref(cost.c), ptr(j["means"]), ptr(j["covs"]), ptr(U), ptr(c), ptr(dm), ptr(dS), ptr(dU),
                                stream_ptr()), "gpmpc_cost_grad")
    gU = linearised_fc_vjp(j["jac"], dm, dS, ds, da)
    gU = (gU[0] if isinstance(gU, (tuple, list)) else gU) + dU
    torch.cuda.synchronize()
    for b in range(B):
        got, want = gU[b].cpu().numpy().reshape(-1), r["grad"][b].cpu().numpy().reshape(-1)
        print("  %s %s [%d]: packed sweep against the rollout's gradient: relative error in norm %.3e"
              % (tag, form, b, np.linalg.norm(got - want) / np.linalg.norm(want)))
        TC._assert_grad(got, want, "%s %s [%d] adjoint" % (tag, form, b), quiet=True)
    np.testing.assert_allclose(c.cpu().numpy(), r["cost"].cpu().numpy(), rtol=1e-10)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. many steps: H da > 64, several waves of the sweep, every element stored
# ------------------------------------------------------------------------------------------------------------------------------
def _tiny(G, N=40, ds=2, da=2, H=40, B=3):
    from gaussian_process_mpc_amd.synth import synth_problem
    from oracle import gpmpc_oracle as O
    pb = synth_problem(1, N, ds, da, H, B)
    gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"])
    pack = G.GPPack(pb["X"], pb["Y"], gp.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"], fullcov=True)
    cost = G.CostParams(-1.0, pb["Q"], pb["R"], x_ref=pb["x_ref"], u_ref=pb["u_ref"])
    return pb, gp, pack, cost


def _raw_constrained(pack, x0, U, cost, sc, grad, fill=float("nan")):
    """gpmpc_rollout_fullcov_constrained into buffers pre-filled with NaN (a store the kernels miss shows), trajectory kept in the workspace."""
    from gaussian_process_mpc_amd import _lib
    from gaussian_process_mpc_amd._lib import lib, ptr, stream_ptr
    dev = pack.device
    x0 = torch.as_tensor(np.ascontiguousarray(x0), device=dev)
    U = torch.as_tensor(np.ascontiguousarray(U), device=dev)
    B, H, da = U.shape
    e = lambda *s: torch.full(s, fill, dtype=torch.float64, device=dev)  # noqa: E731
    out = {"cost": e(B), "g": e(B, H, sc.m), "grad": e(B, H, da), "g_jac": e(B, H * sc.m, H * da)}
    flags = _lib.WANT_GRAD if grad else 0
    ws = pack.workspace(lib().gpmpc_rollout_fullcov_constrained_workspace_bytes(pack.handle, B, H, flags))
    rc = lib().gpmpc_rollout_fullcov_constrained(pack.handle, B, H, ptr(x0), ptr(U), ctypes.byref(cost.c), ctypes.byref(sc.c), flags, None, None,
                                                 ptr(out["cost"]), ptr(out["grad"]) if grad else None, ptr(out["g"]),
                                                 ptr(out["g_jac"]) if grad else None, ctypes.c_void_p(ws.data_ptr()), ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    return rc, out


def test_many_steps_complete_stores_and_causality(G):
    pb, gp, pack, cost = _tiny(G)
    ds, da, H, B = 2, 2, 40, 3
    assert H * da > 64
    A, bb, kap = TC._rows(ds)
    sc = G.StateConstraints(A, bb, kappa=kap)
    rc, out = _raw_constrained(pack, pb["x0"], pb["U"], cost, sc, True)
    assert rc == 0
    for k, t in out.items():
        assert bool(torch.isfinite(t).all()), k                # every element written
    gj = out["g_jac"].cpu().numpy()
    for t in range(1, H + 1):
        blk = gj[:, (t - 1) * 3:t * 3, t * da:]
        assert not np.any(blk) and not np.any(np.signbit(blk)), t
        assert np.all(np.abs(gj[:, (t - 1) * 3:t * 3, (t - 1) * da:t * da]).max(axis=(1, 2)) > 0), t      # the newest input reaches step t
    rc, val = _raw_constrained(pack, pb["x0"], pb["U"], cost, sc, False)
    assert rc == 0 and _same(val["g"], out["g"]) and bool(torch.isnan(val["g_jac"]).all()) and bool(torch.isnan(val["grad"]).all())
    r = G.rollout_fullcov(pack, pb["x0"], pb["U"], cost, want_grad=True, constraints=sc)
    for k in ("cost", "grad", "g", "g_jac"):
        assert _same(r[k], out[k]), k
    # the reference on the last rows of trajectory 0, where 39 steps of the sweep have gone by: values, and rows by the gradient criterion
    ref = F.reference_fullcov_constraints(gp, H, pb["x0"][0], pb["U"][0], A, bb, kap, want_jac=False)
    _assert_g(out["g"][0].cpu().numpy(), ref, A, kap, "tiny H = 40")
    Ut = torch.as_tensor(pb["U"][0]).clone().requires_grad_(True)
    from oracle import gpmpc_oracle as O
    means, covs = O.forward_propagate_fullcov(gp, H, torch.as_tensor(pb["x0"][0]), Ut, "o2")
    g = F.g_of_full_trajectory(means, covs, A, bb, kap)
    for t, row in ((H - 1, 1), (H // 2, 0)):
        (want,) = torch.autograd.grad(g[t, row], Ut, retain_graph=True)
        TC._assert_grad(gj[0, t * 3 + row], want.reshape(-1).numpy(), "tiny row (%d, %d)" % (t, row), quiet=True)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. noise model: a full init_cov and a process variance reach g
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_noise_model_values(G, form):
    tag = "c1"
    pb, gp = TC._problem(tag)
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    A, bb, kap = TC._rows(ds)
    sc, cost = TC._sc(G, ds), TC._cost(G, tag)
    pack = G.GPPack(pb["X"], pb["Y"], gp.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"], fullcov=True)
    P, av, pv = NR.ladder_noise(ds, da)
    assert abs(P[0, 1]) > 1e-4 and pv.min() > 0
    kw = dict(init_cov=P, action_var=av, process_var=pv)
    pack.set_noise(**kw)
    B = 2
    with _tuning(pack, {"GPMPC_FC_FORM": FORMS[form]}):
        assert pack.plan_fullcov(B, H, want_grad=False)["form"] == form
        v = G.rollout_fullcov(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=False, constraints=sc)
        r = G.rollout_fullcov(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=True, constraints=sc)
    assert _same(v["g"], r["g"])
    for b in range(B):
        ref = F.reference_fullcov_constraints(gp, H, pb["x0"][b], pb["U"][b], A, bb, kap, want_jac=False, noise=kw)
        np.testing.assert_allclose(v["covs"][b].cpu().numpy(), ref["covs"], rtol=1e-4, atol=1e-6 * np.abs(ref["covs"]).max())
        _assert_g(v["g"][b].cpu().numpy(), ref, A, kap, "noise %s [%d]" % (form, b))
        # the model matters: the default model's g is far outside the bound
        assert (np.abs(_ref(tag, b)["g"] - ref["g"]) / F.g_tolerance(ref, A, kap)).max() > 50.0


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the solvers equal their chains of public steps, bit for bit; the existing entries keep theirs
# ------------------------------------------------------------------------------------------------------------------------------
def _c1(G):
    pb, _ = TC._problem("c1")
    return pb, _pack(G, "c1"), TC._cost(G, "c1"), pb["x0"][0], pb["H"], pb["da"]


def _evaluate(G, full, pack, x0, U, cost, sc, grad):
    if full:
        return G.rollout_fullcov(pack, x0, U, cost, want_grad=grad, constraints=sc)
    return G.rollout(pack, x0, U, cost, want_grad=grad, want_traj=False, constraints=sc)


@pytest.mark.parametrize("constrained", [False, True])
@pytest.mark.parametrize("full", [True, False], ids=["fullcov", "diagonal"])
def test_mppi_solve_equals_its_parts(G, full, constrained):
    from gaussian_process_mpc_amd.mppi import mppi_sample, mppi_solve, mppi_start, mppi_update
    pb, pack, cost, x0, H, da = _c1(G)
    sc = TC._sc(G, 2) if constrained else None
    K, iters = 16, 3
    opt = dict(sigma=0.5, decay=0.9, beta=0.1, seed=3, call_index=2, lb=-1.0, ub=1.0)
    whole = mppi_solve(pack, x0, np.zeros((H, da)), cost, constraints=sc, samples=K, iterations=iters, full_covariance=full, **opt)
    mean = torch.zeros((H, da), dtype=torch.float64, device="cuda")
    best, trace = mppi_start(mean), []
    for it in range(iters):
        U = mppi_sample(mean, K, opt["sigma"], opt["lb"], opt["ub"], seed=opt["seed"], call_index=opt["call_index"], iteration=it, decay=opt["decay"])
        r = _evaluate(G, full, pack, x0, U, cost, sc, False)
        up = mppi_update(U, r["cost"], best, opt["beta"], g=r.get("g"), mean=mean)
        mean, best = up["mean"], up["best"]
        trace.append(up["trace"].cpu().numpy())
    best = best.cpu().numpy()
    assert _same(whole["trace"], np.array(trace)) and _same(whole["U"].reshape(-1), best[2:])
    assert (whole["violation"], whole["cost"]) == (best[0], best[1])
    if full:                                                 # ... and it is another search than the diagonal one
        other = mppi_solve(pack, x0, np.zeros((H, da)), cost, constraints=sc, samples=K, iterations=iters, **opt)
        assert not _same(other["trace"], whole["trace"])


def _keep(log):
    def callback(*a):
        log.append(tuple(x.clone() if isinstance(x, torch.Tensor) else x for x in a))
    return callback


@pytest.mark.parametrize("full", [True, False], ids=["fullcov", "diagonal"])
def test_lbfgs_solve_equals_its_parts(G, full):
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_solve, lbfgs_start, lbfgs_state_layout, lbfgs_state_view, lbfgs_tick
    from gaussian_process_mpc_amd.multistart import make_starts
    pb, pack, cost, x0, H, da = _c1(G)
    K, m, T = 4, 8, 4
    n = H * da
    X0 = make_starts(K, n, np.full(n, -1.0), np.full(n, 1.0), np.random.default_rng([0, 0]))
    total = lbfgs_state_layout(K, n, m)["total"]
    kw = dict(lb=-1.0, ub=1.0, history=m, gtol=1e-4, ftol=1e-10)
    log = []
    U1, c1, info = lbfgs_solve(pack, x0, X0.reshape(K, H, da), cost, max_ticks=T, check_every=2, callback=_keep(log), full_covariance=full, **kw)
    Xd = torch.as_tensor(X0.reshape(K, H, da), device="cuda")
    state = lbfgs_start(Xd, **kw)
    v = lbfgs_state_view(state, K, H, da, m)
    r = _evaluate(G, full, pack, x0, v["U"], cost, None, True)
    lbfgs_start(Xd, r["cost"], r["grad"], state=state, **kw)
    for _ in range(T):
        r = _evaluate(G, full, pack, x0, v["U"], cost, None, True)
        lbfgs_tick(state, r["cost"], r["grad"], K, H, da, full_covariance=full, **kw)
    assert _same(state[:total], log[-1][1][:total]) and _same(U1, v["plan"])
    assert c1 == float(state[2].item()) and info["ticks"] == T
    if full:
        U0, _, _ = lbfgs_solve(pack, x0, X0.reshape(K, H, da), cost, max_ticks=T, check_every=2, **kw)
        assert not _same(U0, U1)


@pytest.mark.parametrize("full", [True, False], ids=["fullcov", "diagonal"])
def test_auglag_solve_equals_its_parts(G, full):
    from gaussian_process_mpc_amd.device_auglag import auglag_merit, auglag_outer, auglag_solve, auglag_state_layout, auglag_state_new, auglag_state_view
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_start, lbfgs_state_layout, lbfgs_state_view, lbfgs_tick
    from gaussian_process_mpc_amd.multistart import make_starts
    pb, pack, cost, x0, H, da = _c1(G)
    sc = TC._sc(G, 2)
    K, m, T, NO = 4, 8, 3, 2
    n = H * da
    X0 = make_starts(K, n, np.full(n, -1.0), np.full(n, 1.0), np.random.default_rng([0, 0]))
    ta, tl = auglag_state_layout(K, n, H * sc.m)["total"], lbfgs_state_layout(K, n, m)["total"]
    lkw = dict(lb=-1.0, ub=1.0, history=m, gtol=1e-6, ftol=1e-12)
    log = []
    U1, c1, info = auglag_solve(pack, x0, X0.reshape(K, H, da), cost, sc, outer=NO, inner_ticks=T, check_outer=0, callback=_keep(log),
                                full_covariance=full, **lkw)
    Xd = torch.as_tensor(X0.reshape(K, H, da), device="cuda")
    al = auglag_state_new(Xd, 10.0, sc.m, lb=-1.0, ub=1.0)
    va = auglag_state_view(al, K, H, da, sc.m)
    inner = lbfgs_start(Xd, **lkw)
    vi = lbfgs_state_view(inner, K, H, da, m)
    okw = dict(lkw, inner_ticks=T)
    ev = lambda: _evaluate(G, full, pack, x0, vi["U"], cost, sc, True)      # noqa: E731
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
    ws = log[-1][1]
    assert _same(al[:ta], ws[:ta]) and _same(inner[:tl], ws[ta:ta + tl]) and _same(U1, va["plan"])
    assert c1 == float(al[3].item()) and info["best"] == int(al[1].item())


# ------------------------------------------------------------------------------------------------------------------------------
# 7. RiskSensitiveMPC under propagation = "moment_matching_full"
# ------------------------------------------------------------------------------------------------------------------------------
def test_mpc_moment_matching_full(G):
    mpc, gp, pb = TC._mpc_c1(G)
    H, da, ds, x0 = pb["H"], pb["da"], pb["ds"], pb["x0"][0]
    mpc.propagation = "moment_matching_full"
    assert mpc.full_covariance is False
    # the unconstrained solve runs on the full-covariance rollout: its callbacks are rollout_fullcov's numbers
    U_free = mpc.get_optimal_trajectory(x0).copy()
    pack, cp = mpc.dynamics.pack(), mpc._cost_params()
    x = pb["U"][0].reshape(-1).copy()
    one = G.rollout_fullcov(pack, x0, pb["U"][:1], cp, want_grad=True)
    assert mpc.objective(x) == one["cost"][0].item() and _same(np.asarray(mpc.gradient(x)), one["grad"][0])
    assert mpc.constraints(x) == 0
    # a coupled row, active along the unconstrained optimum: b = top - 0.3 span of g(b = 0) under the CPU reference
    A, kap = np.array([[1.0, 0.6]]), np.array([TC.K95])
    along = F.reference_fullcov_constraints(gp, H, x0, U_free, A, [0.0], kap, want_jac=False)["g"][:, 0]
    b = along.max() - 0.3 * (along.max() - along.min())
    mpc.set_state_constraints(A, [b], prob=0.95)
    np.testing.assert_allclose(mpc.state_constraints.kappa, kap, rtol=1e-12)
    kap = mpc.state_constraints.kappa
    rf = lambda U: F.reference_fullcov_constraints(gp, H, x0, U, A, [b], kap, want_jac=False)      # noqa: E731
    free = rf(U_free)
    assert free["g"].max() > 50 * F.g_tolerance(free, A, kap).max()           # otherwise the test shows nothing
    # callbacks against row 0 of the batched screen
    g, jac = mpc.constraints(x), mpc.jacobian(x)
    scr = mpc.evaluate_batch(pb["U"][:3], x0, constraints=True)
    assert tuple(scr["g"].shape) == (3, H, 1) and tuple(scr["g_jac"].shape) == (3, H, H * da) and tuple(scr["covs"].shape) == (3, H + 1, ds, ds)
    assert _same(scr["g"][0].reshape(-1), g) and _same(scr["g_jac"][0].reshape(-1), jac)
    assert "g_jac" not in mpc.evaluate_batch(pb["U"][:3], x0, want_grad=False, constraints=True)
    assert "g" not in mpc.evaluate_batch(pb["U"][:3], x0) and "covs" in mpc.evaluate_batch(pb["U"][:3], x0)
    # the gradient solve
    U_con = mpc.get_optimal_trajectory(x0)
    info = mpc.last_solve_info
    print("constrained: %s %s" % (mpc.solver_used, info))
    if mpc.solver_used == "scipy-slsqp":
        assert info["success"] and info["max_violation"] <= 1e-6, info
    ref = rf(U_con)
    print("  reference max g %.3e, bound %.3e: largest g - bound %.3e" % (ref["g"].max(), F.g_tolerance(ref, A, kap).min(),
                                                                         (ref["g"] - F.g_tolerance(ref, A, kap)).max()))
    assert np.all(ref["g"] <= F.g_tolerance(ref, A, kap))      # feasible under the reference, the margin the tolerance of g
    assert np.all(np.abs(U_con) <= 1.0 + 1e-9)
    # the device solvers on the new entries
    mpc.solver_used, mpc._solve_count = None, 0
    mpc.mppi_options.update(samples=16, iterations=40, sigma=0.5)
    U_m = mpc.get_optimal_trajectory(x0, solver="mppi")
    print("  mppi: %s" % {k: v for k, v in mpc.last_solve_info.items() if k != "trace"})
    assert mpc.solver_used == "mppi x16" and mpc.last_solve_info["feasible"]
    ref = rf(U_m)
    assert np.all(ref["g"] <= F.g_tolerance(ref, A, kap))
    mpc.solver_used, mpc._solve_count = None, 0
    mpc.n_starts = 4
    mpc.auglag_options.update(outer=6, inner_ticks=15)
    U_a = mpc.get_optimal_trajectory(x0, solver="auglag")
    info = mpc.last_solve_info
    print("  auglag: f %s violation %s best %d" % (info["f"], info["violation"], info["best"]))
    assert mpc.solver_used == "device-auglag x4" and info["success"]
    ref = rf(U_a)
    print("  auglag: reference max g %.3e, feas_tol %.1e" % (ref["g"].max(), mpc.auglag_options["feas_tol"]))
    assert ref["g"].max() <= mpc.auglag_options["feas_tol"]    # feasible under the reference to feas_tol
    # refusals under the rule
    with pytest.raises(NotImplementedError, match="moment_matching_full"):
        mpc.get_optimal_trajectory(x0, n_starts=4)
    mpc.n_starts = 1
    mpc.set_feedback_gain(np.zeros((da, ds)))
    with pytest.raises(ValueError, match="feedback gain"):
        mpc.evaluate_batch(pb["U"][:2], x0)
    mpc.clear_feedback_gain()
    nom = G.RiskSensitiveMPC(pb["gamma"], H, ds, da, pb["Q"], pb["R"], nominal_models=G.LinearNominalModel.identity(ds, da))
    nom.propagation = "moment_matching_full"
    with pytest.raises(NotImplementedError, match="nominal model"):
        nom.evaluate_batch(pb["U"][:2], x0)
    # without constraints: the device L-BFGS and the host multi-start, and validate_plan's covariance
    mpc.clear_state_constraints()
    mpc.multistart_options.update(max_ticks=4)
    plan = mpc.get_optimal_trajectory(x0, solver="lbfgs", n_starts=4)
    assert plan.shape == (H, da) and mpc.solver_used == "device-lbfgs x4" and np.all(np.isfinite(plan))
    plan = mpc.get_optimal_trajectory(x0, n_starts=2)
    assert plan.shape == (H, da) and mpc.solver_used == "lockstep-lbfgs x2" and np.all(np.isfinite(plan))
    rep = mpc.validate_plan(plan, x0, particles=256)
    assert rep["cov_mm"].shape == (H + 1, ds, ds) and np.abs(rep["cov_mm"][-1, 0, 1]) > 0
    # back under "moment_matching": the refusals with full_covariance=True raise as before
    mpc.propagation = "moment_matching"
    mpc.set_state_constraints(A, [b], prob=0.95)
    mpc.full_covariance = True
    mpc.curr_state = torch.tensor(x0, dtype=torch.float64, device=mpc.device)
    for call in (lambda: mpc.get_optimal_trajectory(x0), lambda: mpc.evaluate_batch(pb["U"][:2], x0, constraints=True),
                 lambda: mpc.constraints(np.zeros(H * da)), lambda: mpc.get_optimal_trajectory(x0, solver="mppi"),
                 lambda: mpc.get_optimal_trajectory(x0, solver="auglag")):
        with pytest.raises(NotImplementedError, match="full-covariance"):
            call()
    mpc.clear_state_constraints()
    with pytest.raises(NotImplementedError, match="full-covariance"):
        mpc.get_optimal_trajectory(x0, solver="lbfgs")
    mpc.full_covariance = False


# ------------------------------------------------------------------------------------------------------------------------------
# 8. refusals of the C entries: before any launch, with text
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(G):
    from gaussian_process_mpc_amd import _lib
    from gaussian_process_mpc_amd._lib import lib
    from nominal_reference import synth_nominal
    pb, gp = TC._problem("c1")
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    cost = TC._cost(G, "c1")
    A, bb, kap = TC._rows(ds)
    sc = G.StateConstraints(A, bb, kappa=kap)
    good = _pack(G, "c1")
    text = lambda: lib().gpmpc_last_error().decode()         # noqa: E731

    def untouched(out):
        return all(bool(torch.isnan(t).all()) for t in out.values())

    # a pack without cross-covariance weights, a pack with a nominal model, a pack that is not built
    bare = G.GPPack(pb["X"], pb["Y"], gp.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"])
    rc, out = _raw_constrained(bare, pb["x0"][:2], pb["U"][:2], cost, sc, True)
    assert rc == -5 and "gpmpc_rollout_fullcov_constrained" in text() and "cross-covariance weights" in text() and untouched(out)
    # the text belongs to the entry that set it: the older entry, which sets none for this state, never shows a stale one
    with pytest.raises(G.GpmpcError, match="cross-covariance weights"):
        _lib.check(-5, "gpmpc_rollout_fullcov_constrained")
    with pytest.raises(G.GpmpcError) as stale:
        _lib.check(-5, "gpmpc_rollout_fullcov")
    assert "cross-covariance" not in str(stale.value)
    nominal = G.GPPack(pb["X"], pb["Y"], gp.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"], nominal=synth_nominal(ds, da))
    rc, out = _raw_constrained(nominal, pb["x0"][:2], pb["U"][:2], cost, sc, True)
    assert rc == -5 and "nominal model" in text() and untouched(out)
    with pytest.raises(NotImplementedError, match="nominal"):
        G.rollout_fullcov(nominal, pb["x0"][:2], pb["U"][:2], cost, constraints=sc)
    with pytest.raises(NotImplementedError, match="nominal"):
        G.rollout_fullcov_jac(nominal, pb["x0"][:2], pb["U"][:2])
    h = ctypes.c_void_p()
    assert lib().gpmpc_pack_create(ctypes.byref(h), 10, 2, 2) == 0
    try:
        fake = ctypes.c_void_p(4096)
        rc = lib().gpmpc_rollout_fullcov_constrained(h, 1, 4, fake, fake, ctypes.byref(cost.c), ctypes.byref(sc.c), _lib.WANT_GRAD, None, None,
                                                     fake, fake, fake, fake, fake, 1 << 20, None)
        assert rc == -5 and "not built" in text()
        assert lib().gpmpc_rollout_fullcov_jac(h, 1, 4, fake, fake, fake, fake, fake, fake, 1 << 20, None) == -5
    finally:
        lib().gpmpc_pack_destroy(h)
    # the rows, the flags, the cost schedule
    bad = G.StateConstraints(A, bb, kappa=kap)
    bad.c.kappa[1] = -1.0
    rc, out = _raw_constrained(good, pb["x0"][:2], pb["U"][:2], cost, bad, True)
    assert rc == -1 and "kappa[1]" in text() and untouched(out)
    bad.c.kappa[1], bad.c.n_rows = 2.0, 17
    rc, out = _raw_constrained(good, pb["x0"][:2], pb["U"][:2], cost, bad, False)
    assert rc == -1 and "n_rows" in text() and untouched(out)
    x0d, Ud = (torch.as_tensor(np.ascontiguousarray(a), device=good.device) for a in (pb["x0"][:2], pb["U"][:2]))
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=good.device)      # noqa: E731
    ws = good.workspace(lib().gpmpc_rollout_fullcov_constrained_workspace_bytes(good.handle, 2, H, _lib.WANT_GRAD))

    def call(cost_c, flags, nbytes=None):
        out = {"cost": nan(2), "grad": nan(2, H, da), "g": nan(2, H, 3), "g_jac": nan(2, H * 3, H * da)}
        rc = lib().gpmpc_rollout_fullcov_constrained(good.handle, 2, H, _lib.ptr(x0d), _lib.ptr(Ud), ctypes.byref(cost_c), ctypes.byref(sc.c), flags,
                                                     None, None, _lib.ptr(out["cost"]), _lib.ptr(out["grad"]), _lib.ptr(out["g"]),
                                                     _lib.ptr(out["g_jac"]), ctypes.c_void_p(ws.data_ptr()), ws.numel() if nbytes is None else nbytes,
                                                     _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, out
    for flags in (_lib.WANT_GRAD | _lib.USE_GRAPH, _lib.FP32_ACCUM, 64):
        rc, out = call(cost.c, flags)
        assert rc == -1 and "gpmpc_rollout_fullcov_constrained" in text() and untouched(out), flags
    assert lib().gpmpc_rollout_fullcov_constrained_workspace_bytes(good.handle, 2, H, _lib.USE_GRAPH) == 0
    ghost = G.CostParams(pb["gamma"], pb["Q"], pb["R"])
    ghost.c.schedule_id = 987654
    rc, out = call(ghost.c, _lib.WANT_GRAD)
    assert rc == -1 and "cost schedule" in text() and untouched(out)
    rc, out = call(cost.c, _lib.WANT_GRAD, nbytes=1024)
    assert rc == -4 and untouched(out)
    rc, out = call(cost.c, _lib.WANT_GRAD)
    assert rc == 0 and not any(bool(torch.isnan(t).any()) for t in out.values())
    # what the cost kernel cannot take is refused BEFORE the rollout is enqueued, and does not bind the entry that runs no cost kernel: a
    # horizon beyond the kernel's LDS (ds = 2, da = 2: H > 671) ...
    Hl = 700
    assert lib().gpmpc_rollout_fullcov_workspace_bytes(good.handle, 1, Hl, _lib.WANT_GRAD) > 0
    Ul = 0.1 * np.random.default_rng(4).standard_normal((1, Hl, da))
    rc, out = _raw_constrained(good, pb["x0"][:1], Ul, cost, sc, True)
    assert rc == -1 and "gpmpc_rollout_fullcov_constrained" in text() and "LDS" in text() and untouched(out)
    rc, out = _raw_constrained(good, pb["x0"][:1], Ul, cost, sc, False)
    assert rc == -1 and "LDS" in text() and untouched(out)
    jl = G.rollout_fullcov_jac(good, pb["x0"][:1], Ul)
    assert tuple(jl["jac"].shape) == (1, Hl, 5, 7) and bool(torch.isfinite(jl["jac"]).all()) and bool(torch.isfinite(jl["covs"]).all())
    from gaussian_process_mpc_amd.mppi import mppi_params
    Pl = mppi_params(4, da, 0.5, iterations=1)
    wsl = good.workspace(max(int(lib().gpmpc_mppi_solve_fullcov_workspace_bytes(good.handle, Hl, ctypes.byref(Pl), None)), 256))
    resl, Uld = nan(Hl * da + 2 + 6), torch.as_tensor(np.ascontiguousarray(Ul[0]), device=good.device)
    rc = lib().gpmpc_mppi_solve_fullcov(good.handle, Hl, _lib.ptr(x0d[0].contiguous()), _lib.ptr(Uld), ctypes.byref(cost.c), None, ctypes.byref(Pl),
                                        _lib.ptr(resl[:Hl * da]), _lib.ptr(resl[Hl * da:Hl * da + 2]), _lib.ptr(resl[Hl * da + 2:]),
                                        ctypes.c_void_p(wsl.data_ptr()), wsl.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and "gpmpc_mppi_solve_fullcov" in text() and "LDS" in text() and bool(torch.isnan(resl).all())
    # ... and a state dimension the rollout's cost kernel is not built for (ds = 7, da = 1): no entry takes it
    from gaussian_process_mpc_amd.synth import synth_problem
    from oracle import gpmpc_oracle as O
    p7 = synth_problem(4, 40, 7, 1, 3, 2)
    g7 = O.GPBundle(p7["X"], p7["Y"], p7["lambdas"], p7["sigma_f"], p7["sigma_n"])
    pack7 = G.GPPack(p7["X"], p7["Y"], g7.Ky_inv.numpy(), p7["lambdas"], p7["sigma_f"], fullcov=True)
    cost7 = G.CostParams(-1.0, p7["Q"], p7["R"], x_ref=p7["x_ref"], u_ref=p7["u_ref"])
    sc7 = G.StateConstraints(np.ones((1, 7)), 1.0, kappa=1.0)
    rc, out = _raw_constrained(pack7, p7["x0"], p7["U"], cost7, sc7, True)
    assert rc == -1 and "state_dim <= 6" in text() and untouched(out)
    with pytest.raises(G.GpmpcError, match="state_dim <= 6"):
        G.rollout_fullcov_jac(pack7, p7["x0"], p7["U"])
    # the solvers' own refusal of a pack without the weights
    P = mppi_params(8, da, 0.5, iterations=1)
    wsb = bare.workspace(1 << 22)
    res = nan(H * da + 2 + 6)
    rc = lib().gpmpc_mppi_solve_fullcov(bare.handle, H, _lib.ptr(x0d[0].contiguous()), _lib.ptr(Ud[0].contiguous()), ctypes.byref(cost.c), None,
                                        ctypes.byref(P), _lib.ptr(res[:H * da]), _lib.ptr(res[H * da:H * da + 2]), _lib.ptr(res[H * da + 2:]),
                                        ctypes.c_void_p(wsb.data_ptr()), wsb.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -5 and "gpmpc_mppi_solve_fullcov" in text() and bool(torch.isnan(res).all())
