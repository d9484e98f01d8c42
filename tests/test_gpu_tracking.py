"""GPU tests of the cost schedule -- time-varying references x_ref[t], u_ref[t] and a terminal weight Q_f -- through every cost kernel
(step_tail.hip, fullcov.hip, cost.hip) and every entry that takes cost parameters, against the float64 CPU reference of
tests/tracking_reference.py (the pinned oracle + autograd, none of the kernels' closed forms).

Tolerances are the project's: cost 1e-6 relative, gradients 1e-4 relative along the reference gradient and three seeded directions and in
norm (tests/test_gpu_nominal.py::_assert_grad), 1e-12 relative where two device paths are compared, bits where one path is run twice.
The references sit an O(1) distance from the plans' means (tracking_reference.offset_references), so every cost is O(1): asserted on the
CPU reference before anything is compared."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import tracking_reference as T
from nominal_reference import synth_nominal

pytestmark = pytest.mark.gpu

COST_RTOL, GRAD_RTOL = 1e-6, 1e-4
N = 48
_cache = {}


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    return g


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


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)).view(np.uint64)


def _problem(ds, da, H, B, n=N, cfg=None):
    """synth_problem + oracle bundle + one set of references for the whole batch (offset from trajectory 0's means), cached per module."""
    key = (ds, da, H, B, n)
    if key not in _cache:
        from gaussian_process_mpc_amd.synth import synth_problem
        from oracle import gpmpc_oracle as O
        pb = synth_problem(10 * ds + da if cfg is None else cfg, n, ds, da, H, B)
        gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"])
        base = T.tracking_objective(gp, H, pb["x0"][0], pb["U"][0], np.zeros((H + 1, ds)), None, pb["Q"], pb["R"], -1.0, want_grad=False)
        Xr, Ur = T.offset_references(base["means"], pb["U"][0], 100 + ds, offset=1.0 if H < 20 else 0.7)
        _cache[key] = (pb, gp, Xr, Ur, T.general_weight(ds, 50 + ds))
    return _cache[key]


def _pack(G, pb, gp, **kw):
    return G.GPPack(pb["X"], pb["Y"], gp.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"], **kw)


def _variants(pb, Xr, Ur, Qf, rdelta_case=True):
    """gamma x terminal weight x input references, and R_delta on in one case."""
    out = []
    for gamma in (1e-5, -1.0, 0.0):
        for qf in (None, Qf):
            for ur in (None, Ur):
                out.append(dict(X_ref=Xr, U_ref=ur, Q=pb["Q"], gamma=gamma, Q_terminal=qf))
    if rdelta_case:
        out.append(dict(X_ref=Xr, U_ref=Ur, Q=pb["Q"], gamma=-1.0, Q_terminal=Qf, R_delta=0.05 * np.eye(pb["da"]),
                        last_u=np.full(pb["da"], 0.3)))
    return out


def _name(v):
    return "gamma=%g Qf=%d Uref=%d Rd=%d" % (v["gamma"], v["Q_terminal"] is not None, v["U_ref"] is not None, "R_delta" in v)


def _refs(key, gp, pb, H, pick, variants, **kw):
    """refs[b][k] = dict(cost, grad) of trajectory b under variant k: one CPU rollout per trajectory, computed once per module."""
    if ("ref",) + key not in _cache:
        out = {}
        for b in pick:
            r, means, covs = T.tracking_objectives(gp, H, pb["x0"][b], pb["U"][b], pb["R"], variants, **kw)
            assert np.all(np.isfinite(means)) and np.all(np.diagonal(covs, axis1=1, axis2=2) > 0), (key, b)
            for v, rv in zip(variants, r):      # neither cancelled to nothing nor blown up: a relative tolerance means something
                assert np.isfinite(rv["cost"]) and 0.05 < rv["cost"] < 100.0 and np.linalg.norm(rv["grad"]) > 1e-3, (key, b, _name(v), rv["cost"])
            out[b] = r
        _cache[("ref",) + key] = out
    return _cache[("ref",) + key]


def _assert_grad(got, ref, what):
    """The project's gradient criterion (tests/test_gpu_nominal.py::_assert_grad)."""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    rng = np.random.default_rng(12345)
    dirs = [ref / np.linalg.norm(ref)] + [d / np.linalg.norm(d) for d in rng.standard_normal((3, ref.size))]
    for k, d in enumerate(dirs):
        a, e = float(got @ d), float(ref @ d)
        assert abs(a - e) <= GRAD_RTOL * abs(e), (what, k, a, e)
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    assert err <= GRAD_RTOL, (what, err)
    return err


def _cost_of(G, pb, v, cs):
    kw = dict(R_delta=v["R_delta"], last_u=v["last_u"]) if "R_delta" in v else {}
    return G.CostParams(v["gamma"], v["Q"], pb["R"], schedule=cs, x_ref=np.full(pb["ds"], 9.0), u_ref=np.full(pb["da"], -9.0), **kw)   # (ignored)


def _check(r, refs, pick, k, what):
    cost, grad = r["cost"].cpu().numpy(), r["grad"].cpu().numpy()
    assert np.all(np.isfinite(cost)) and np.all(np.isfinite(grad)), what
    worst_c = max(abs(cost[b] - refs[b][k]["cost"]) / abs(refs[b][k]["cost"]) for b in pick)
    worst_g = max(np.linalg.norm(grad[b] - refs[b][k]["grad"]) / np.linalg.norm(refs[b][k]["grad"]) for b in pick)
    print("DEV %s: cost %.3g grad %.3g of the tolerance" % (what, worst_c / COST_RTOL, worst_g / GRAD_RTOL))
    for b in pick:
        np.testing.assert_allclose(cost[b], refs[b][k]["cost"], rtol=COST_RTOL, err_msg=what)
        _assert_grad(grad[b], refs[b][k]["grad"], "%s [%d]" % (what, b))


# ------------------------------------------------------------------------------------------------------------------------------
# 1. against the reference
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds,da,H,B", [(2, 1, 4, 3), (3, 2, 5, 1), (4, 1, 6, 70)])
def test_rollout_against_the_reference(G, ds, da, H, B):
    """Cost and gradient under gamma in {1e-5, -1, 0} x with / without a non-symmetric Q_f x with / without U_ref, R_delta on in one case.
    B = 70 also as the whole-horizon kernel (the tail starts from `finished`; at N = 48 the planner's cost comparison takes that form from
    B ~ 108 on, so it is asked for, as tests/test_gpu_offgrid.py does, and asserted from the plan) and under GPMPC_PERSIST=0."""
    pb, gp, Xr, Ur, Qf = _problem(ds, da, H, B)
    pick = sorted({0, B // 2, B - 1})
    variants = _variants(pb, Xr, Ur, Qf)
    refs = _refs((ds, da, H, B), gp, pb, H, pick, variants)
    pack = _pack(G, pb, gp)
    cs = G.CostSchedule(H + 2, ds, da)                       # (H_max above the horizon: the offsets come from H_max, the rows from H)
    envs = [({}, None)] + ([({"GPMPC_PERSIST": "16"}, "persist"), ({"GPMPC_PERSIST": "0"}, "not persist")] if B == 70 else [])
    for env, form in envs:
        with _tuning(pack, env):
            plan = pack.plan(B, H)
            print("plan B=%d %s: %s" % (B, env, plan))
            if form == "persist":
                assert plan["form"] == "persist", plan
            elif form is not None:
                assert plan["form"] != "persist", plan
            for k, v in enumerate(variants):
                cs.set(v["X_ref"], v["U_ref"], v["Q_terminal"])
                r = G.rollout(pack, pb["x0"], pb["U"], _cost_of(G, pb, v, cs), want_traj=False)
                _check(r, refs, pick, k, "ds=%d da=%d H=%d B=%d %s %s" % (ds, da, H, B, plan["form"], _name(v)))
                f = G.rollout(pack, pb["x0"], pb["U"], _cost_of(G, pb, v, cs), want_grad=False, want_traj=False)     # objective only
                np.testing.assert_array_equal(_bits(f["cost"]), _bits(r["cost"]))
    cs.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the tail that keeps one Jacobian in LDS at a time
# ------------------------------------------------------------------------------------------------------------------------------
def _tail_all_in_lds(H, ds, da):
    """The LDS rule of gpmpc_launch_roll_tail (csrc/step_tail.hip) with the gradient."""
    lds0 = 8 * ((H + 1) * (1 + 2 * ds) + H * da + H)
    return lds0 + 8 * 2 * ds * (2 * ds + da) * H <= 48 * 1024


def test_per_step_tail_variant(G):
    """ds = 6, da = 2: the Jacobians of H = 33 steps fit the 48 KiB of the all-in-LDS tail, those of H = 34 do not.  N = 32 points in
    eight dimensions leave the predicted variances near sigma_f^2: tr(Q Sigma) alone is ~0.6 per step (21 over the horizon) whatever the
    references; they are offset by 0.7, which puts the tracking part at a third of the cost (CPU reference: 32.0 and 35.5)."""
    ds, da, H, B = 6, 2, 34, 2
    assert _tail_all_in_lds(H - 1, ds, da) and not _tail_all_in_lds(H, ds, da)
    pb, gp, Xr, Ur, Qf = _problem(ds, da, H, B, n=32)
    variants = [dict(X_ref=Xr, U_ref=Ur, Q=pb["Q"], gamma=-1.0, Q_terminal=Qf), dict(X_ref=Xr, U_ref=None, Q=pb["Q"], gamma=0.0, Q_terminal=None)]
    refs = _refs((ds, da, H, B, 32), gp, pb, H, [0, 1], variants)         # (asserts: finite, variances positive, cost O(1))
    pack = _pack(G, pb, gp)
    cs = G.CostSchedule(H, ds, da)
    for k, v in enumerate(variants):
        cs.set(v["X_ref"], v["U_ref"], v["Q_terminal"])
        r = G.rollout(pack, pb["x0"], pb["U"], _cost_of(G, pb, v, cs), want_traj=False)
        _check(r, refs, [0, 1], k, "per-step tail H=%d %s" % (H, _name(v)))
    # one step shorter: the all-in-LDS variant on the leading rows of the same schedule, the terminal weight at ITS last step
    v = variants[0]
    cs.set(v["X_ref"], v["U_ref"], v["Q_terminal"])
    r = G.rollout(pack, pb["x0"], pb["U"][:, :H - 1], _cost_of(G, pb, v, cs), want_traj=False)
    ref = T.tracking_objective(gp, H - 1, pb["x0"][0], pb["U"][0][:H - 1], Xr, Ur, pb["Q"], pb["R"], -1.0, Q_terminal=Qf)
    np.testing.assert_allclose(r["cost"][0].item(), ref["cost"], rtol=COST_RTOL)
    _assert_grad(r["grad"][0].cpu().numpy(), ref["grad"], "all-in-LDS tail H=%d" % (H - 1))
    cs.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 3. nominal pack x schedule
# ------------------------------------------------------------------------------------------------------------------------------
def test_nominal_pack_with_a_schedule(G):
    ds, da, H, B = 2, 1, 4, 3
    pb, gp, Xr, Ur, Qf = _problem(ds, da, H, B)
    nom = synth_nominal(ds, da)
    variants = [dict(X_ref=Xr, U_ref=Ur, Q=pb["Q"], gamma=g, Q_terminal=Qf) for g in (-1.0, 0.0)]
    refs = _refs((ds, da, H, B, "nominal"), gp, pb, H, [0, 1, 2], variants, nominal=nom)
    pack = _pack(G, pb, gp, nominal=nom)
    assert pack.plan(B, H).get("nominal") == 1
    cs = G.CostSchedule(H, ds, da)
    for k, v in enumerate(variants):
        cs.set(v["X_ref"], v["U_ref"], v["Q_terminal"])
        _check(G.rollout(pack, pb["x0"], pb["U"], _cost_of(G, pb, v, cs), want_traj=False), refs, [0, 1, 2], k, "nominal " + _name(v))
    cs.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 4. full covariance
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds,da,H,B", [(2, 1, 4, 2), (3, 1, 4, 1)])
def test_fullcov_against_the_fullcov_twin(G, ds, da, H, B):
    pb, gp, Xr, Ur, Qf = _problem(ds, da, H, B)
    pick = list(range(B))
    variants = _variants(pb, Xr, Ur, Qf, rdelta_case=True)
    refs = _refs((ds, da, H, B, "fullcov"), gp, pb, H, pick, variants, fullcov=True)
    pack = _pack(G, pb, gp)
    cs = G.CostSchedule(H, ds, da)
    for k, v in enumerate(variants):
        cs.set(v["X_ref"], v["U_ref"], v["Q_terminal"])
        r = G.rollout_fullcov(pack, pb["x0"], pb["U"], _cost_of(G, pb, v, cs))
        _check(r, refs, pick, k, "fullcov ds=%d B=%d %s" % (ds, B, _name(v)))
    cs.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 5. two kernels, one answer
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [1e-5, -1.0, 0.0])
def test_stand_alone_cost_equals_the_rollouts_cost(G, gamma):
    """gpmpc_cost_grad with the schedule on the rollout's own means and diag(vars) against the tail kernel's cost."""
    from gaussian_process_mpc_amd.autograd import CostFunction
    from gaussian_process_mpc_amd.rollout import cost_full
    ds, da, H, B = 3, 2, 5, 4
    pb, gp, Xr, Ur, Qf = _problem(ds, da, H, B)
    pack = _pack(G, pb, gp)
    cs = G.CostSchedule(H, ds, da).set(Xr, Ur, Qf)
    cost = G.CostParams(gamma, pb["Q"], pb["R"], schedule=cs, R_delta=0.05 * np.eye(da), last_u=np.full(da, 0.3))
    r = G.rollout(pack, pb["x0"], pb["U"], cost)
    U = torch.as_tensor(pb["U"], device="cuda")
    c = CostFunction.apply(r["means"].clone().requires_grad_(True), torch.diag_embed(r["vars"]), U, cost)
    rel = ((c - r["cost"]).abs() / r["cost"].abs()).max().item()
    print("gamma = %g: stand-alone cost against the tail's, relative %.3e" % (gamma, rel))
    assert rel <= 1e-12
    np.testing.assert_array_equal(_bits(cost_full(cost, r["means"], torch.diag_embed(r["vars"]), U)), _bits(c))
    cs.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 6. a constant schedule is no schedule
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [1e-5, -1.0, 0.0])
def test_constant_schedule_is_bit_equal_to_no_schedule(G, gamma):
    from gaussian_process_mpc_amd.autograd import CostFunction
    ds, da, H, B = 3, 2, 5, 4
    pb, gp = _problem(ds, da, H, B)[:2]
    pack = _pack(G, pb, gp)
    xr, ur = np.array([0.3, -0.2, 0.1]), np.array([0.1, -0.4])
    kw = dict(R_delta=0.05 * np.eye(da), last_u=np.full(da, 0.3))
    plain = G.CostParams(gamma, pb["Q"], pb["R"], x_ref=xr, u_ref=ur, **kw)
    cs = G.CostSchedule(H + 3, ds, da)
    sched = G.CostParams(gamma, pb["Q"], pb["R"], schedule=cs, **kw)
    U = torch.as_tensor(pb["U"], device="cuda")
    a = G.rollout(pack, pb["x0"], pb["U"], plain)
    fa = G.rollout_fullcov(pack, pb["x0"], pb["U"], plain)
    for qf in (None, pb["Q"]):                                # a terminal weight equal to Q is no terminal weight either
        cs.set(np.tile(xr, (H + 1, 1)), np.tile(ur, (H, 1)), qf)
        b = G.rollout(pack, pb["x0"], pb["U"], sched)
        for key in ("cost", "grad", "means", "vars"):
            np.testing.assert_array_equal(_bits(a[key]), _bits(b[key]), err_msg=key)
        fb = G.rollout_fullcov(pack, pb["x0"], pb["U"], sched)
        for key in ("cost", "grad"):
            np.testing.assert_array_equal(_bits(fa[key]), _bits(fb[key]), err_msg="fullcov " + key)
        # the stand-alone cost: its schedule variant holds the elimination in registers, the plain kernel in scratch -- the same
        # operations in the same order
        outs = []
        for cp in (plain, sched):
            m = a["means"].clone().requires_grad_(True)
            S = torch.diag_embed(a["vars"]).clone().requires_grad_(True)
            u = U.clone().requires_grad_(True)
            c = CostFunction.apply(m, S, u, cp)
            c.sum().backward()
            outs.append((c, m.grad, S.grad, u.grad))
        for x, y in zip(*outs):
            np.testing.assert_array_equal(_bits(x), _bits(y))
    cs.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 7. indexing
# ------------------------------------------------------------------------------------------------------------------------------
def test_rows_horizons_and_batches(G):
    ds, da, H, B = 4, 1, 6, 70
    pb, gp, Xr, Ur, Qf = _problem(ds, da, H, B)
    pack = _pack(G, pb, gp)
    cs, cs2 = G.CostSchedule(H, ds, da), G.CostSchedule(H, ds, da)
    cost, cost2 = (G.CostParams(-1.0, pb["Q"], pb["R"], schedule=c) for c in (cs, cs2))
    x0, U = pb["x0"][:3], pb["U"][:3]
    cs.set(Xr, Ur, Qf)
    a = G.rollout(pack, x0, U, cost, want_traj=False)
    cs.set(np.roll(Xr, 1, axis=0), Ur, Qf)                    # the rows shifted by one
    b = G.rollout(pack, x0, U, cost, want_traj=False)
    assert np.all(np.abs(a["cost"].cpu().numpy() - b["cost"].cpu().numpy()) > 1e-3)
    # a shorter call: rows 0..H', Q_f at H' -- the schedule set at H' itself, bit for bit
    cs.set(Xr, Ur, Qf)
    for Hs in (1, 3, H - 1):
        cs2.set(Xr[:Hs + 1], Ur[:Hs], Qf)
        s1 = G.rollout(pack, x0, U[:, :Hs], cost, want_traj=False)
        s2 = G.rollout(pack, x0, U[:, :Hs], cost2, want_traj=False)
        for key in ("cost", "grad"):
            np.testing.assert_array_equal(_bits(s1[key]), _bits(s2[key]), err_msg="H'=%d %s" % (Hs, key))
        ref = T.tracking_objective(gp, Hs, x0[0], U[0][:Hs], Xr, Ur, pb["Q"], pb["R"], -1.0, Q_terminal=Qf)
        np.testing.assert_allclose(s1["cost"][0].item(), ref["cost"], rtol=COST_RTOL)
    # a batch of 64 against 64 single calls, under ONE kernel form (plans differ by rounding, DESIGN.md section 5: one workgroup per
    # trajectory of the whole-horizon kernel for both)
    with _tuning(pack, {"GPMPC_PERSIST": "16"}):
        assert pack.plan(64, H)["form"] == "persist" and pack.plan(1, H)["form"] == "persist"
        whole = G.rollout(pack, pb["x0"][:64], pb["U"][:64], cost, want_traj=False)
        wc, wg = whole["cost"].cpu().numpy(), whole["grad"].cpu().numpy()
        for k in range(64):
            one = G.rollout(pack, pb["x0"][k], pb["U"][k], cost, want_traj=False)
            assert _bits(one["cost"])[0] == _bits(wc[k:k + 1])[0], k
            np.testing.assert_array_equal(_bits(one["grad"][0]), _bits(wg[k]))
    cs.close()
    cs2.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 8. graphs
# ------------------------------------------------------------------------------------------------------------------------------
def test_one_capture_serves_every_set(G):
    ds, da, H, B = 2, 1, 4, 3
    pb, gp, Xr, Ur, Qf = _problem(ds, da, H, B)
    pack = _pack(G, pb, gp)
    lib = G.lib()
    cs = G.CostSchedule(H, ds, da)
    cost = G.CostParams(-1.0, pb["Q"], pb["R"], schedule=cs)
    cb0, gr0 = lib.gpmpc_pack_callback_captures(pack.handle), lib.gpmpc_pack_graph_captures(pack.handle)
    seen = set()
    ptr0 = None
    for k in range(5):
        cs.set(Xr + 0.1 * k, Ur if k % 2 else None, Qf if k in (1, 2) else None)
        ptr0 = cs.get()["ptr"] if ptr0 is None else ptr0
        assert cs.get()["ptr"] == ptr0                        # the same device allocation every time
        plain1 = G.rollout(pack, pb["x0"][0], pb["U"][0], cost, want_traj=False)
        cg = pack.objective_gradient(pb["x0"][0], pb["U"][0], cost)
        np.testing.assert_array_equal(_bits(cg[:1]), _bits(plain1["cost"]))
        np.testing.assert_array_equal(_bits(cg[1:]), _bits(plain1["grad"].reshape(-1)))
        plain = G.rollout(pack, pb["x0"], pb["U"], cost, want_traj=False)
        rep = G.rollout(pack, pb["x0"], pb["U"], cost, want_traj=False, graph=True)
        np.testing.assert_array_equal(_bits(rep["cost"]), _bits(plain["cost"]))
        np.testing.assert_array_equal(_bits(rep["grad"]), _bits(plain["grad"]))
        seen.add(float(plain["cost"][0].item()))
    assert len(seen) == 5                                     # every set took effect
    assert lib.gpmpc_pack_callback_captures(pack.handle) == cb0 + 1
    assert lib.gpmpc_pack_graph_captures(pack.handle) == gr0 + 1
    cs.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 9. solvers
# ------------------------------------------------------------------------------------------------------------------------------
def _c1(G):
    if "c1" not in _cache:
        from gaussian_process_mpc_amd.multistart import make_starts
        from gaussian_process_mpc_amd.synth import synth_problem
        from oracle import gpmpc_oracle as O
        pb = synth_problem(1, 100, 2, 2, 10, 64)
        gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"])
        H, x0 = 10, pb["x0"][0]
        base = T.tracking_objective(gp, H, x0, pb["U"][1], np.zeros((H + 1, 2)), None, pb["Q"], pb["R"], 1e-5, want_grad=False)
        n = H * 2
        X0 = make_starts(4, n, np.full(n, -1.0), np.full(n, 1.0), np.random.default_rng([0, 0]))
        assert not X0[0].any()
        _cache["c1"] = (pb, gp, base["means"] + 0.2, X0)
    return _cache["c1"]


def _c1_setup(G):
    pb, gp, Xr, X0 = _c1(G)
    pack = _pack(G, pb, gp)
    Qf = 10.0 * pb["Q"]
    cs = G.CostSchedule(10, 2, 2).set(Xr, None, Qf)
    cost = G.CostParams(1e-5, pb["Q"], pb["R"], schedule=cs)
    rc = lambda U: T.tracking_objective(gp, 10, pb["x0"][0], U, Xr, None, pb["Q"], pb["R"], 1e-5, Q_terminal=Qf, want_grad=False)["cost"]  # noqa: E731
    return pb, pack, cs, cost, rc, X0


def test_mppi_solve_with_a_schedule_equals_its_parts(G):
    from gaussian_process_mpc_amd.mppi import mppi_sample, mppi_solve, mppi_start, mppi_update
    pb, pack, cs, cost, rc, _ = _c1_setup(G)
    x0, H, da, K, iters = pb["x0"][0], 10, 2, 64, 3
    opt = dict(sigma=0.5, decay=0.9, beta=0.1, seed=3, call_index=2, lb=-1.0, ub=1.0)
    whole = mppi_solve(pack, x0, np.zeros((H, da)), cost, samples=K, iterations=iters, **opt)
    mean = torch.zeros((H, da), dtype=torch.float64, device="cuda")
    best, trace = mppi_start(mean), []
    for it in range(iters):
        U = mppi_sample(mean, K, opt["sigma"], opt["lb"], opt["ub"], seed=opt["seed"], call_index=opt["call_index"], iteration=it, decay=opt["decay"])
        r = G.rollout(pack, x0, U, cost, want_grad=False, want_traj=False)
        up = mppi_update(U, r["cost"], best, opt["beta"], mean=mean)
        mean, best = up["mean"], up["best"]
        trace.append(up["trace"].cpu().numpy())
    best = best.cpu().numpy()
    np.testing.assert_array_equal(_bits(whole["trace"]), _bits(np.array(trace)))
    np.testing.assert_array_equal(_bits(whole["U"].reshape(-1)), _bits(best[2:]))
    c_plan, c_start = rc(np.asarray(whole["U"]).reshape(H, da)), rc(np.zeros((H, da)))
    print("mppi: reference cost of the plan %.6f, of the start %.6f" % (c_plan, c_start))
    np.testing.assert_allclose(whole["cost"], c_plan, rtol=COST_RTOL)
    assert c_plan <= c_start
    cs.close()


def test_lbfgs_solve_with_a_schedule_equals_its_parts(G):
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_solve, lbfgs_start, lbfgs_state_layout, lbfgs_state_view, lbfgs_tick
    pb, pack, cs, cost, rc, X0 = _c1_setup(G)
    H, da, x0, K, m, Tn = 10, 2, pb["x0"][0], 4, 8, 6
    total = lbfgs_state_layout(K, H * da, m)["total"]
    kw = dict(lb=-1.0, ub=1.0, history=m, gtol=1e-4, ftol=1e-10)
    log = []
    U1, c1, info1 = lbfgs_solve(pack, x0, X0.reshape(K, H, da), cost, max_ticks=Tn, check_every=0, callback=lambda t, ws: log.append(ws.clone()), **kw)
    Xd = torch.as_tensor(X0.reshape(K, H, da), device="cuda")
    state = lbfgs_start(Xd, **kw)
    v = lbfgs_state_view(state, K, H, da, m)
    r = G.rollout(pack, x0, v["U"], cost, want_grad=True, want_traj=False)
    lbfgs_start(Xd, r["cost"], r["grad"], state=state, **kw)
    for _ in range(Tn):
        r = G.rollout(pack, x0, v["U"], cost, want_grad=True, want_traj=False)
        lbfgs_tick(state, r["cost"], r["grad"], K, H, da, **kw)
    np.testing.assert_array_equal(_bits(state[:total]), _bits(log[-1][:total]))
    np.testing.assert_array_equal(_bits(U1), _bits(v["plan"]))
    c_plan, c_start = rc(np.asarray(U1).reshape(H, da)), rc(np.zeros((H, da)))
    print("lbfgs: reference cost of the plan %.6f, of the zero start %.6f" % (c_plan, c_start))
    np.testing.assert_allclose(c1, c_plan, rtol=COST_RTOL)
    assert c_plan <= c_start
    cs.close()


def test_auglag_solve_with_a_schedule_equals_its_parts(G):
    from gaussian_process_mpc_amd.device_auglag import auglag_merit, auglag_outer, auglag_solve, auglag_state_layout, auglag_state_new, auglag_state_view
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_start, lbfgs_state_layout, lbfgs_state_view, lbfgs_tick
    pb, pack, cs, cost, rc, X0 = _c1_setup(G)
    sc = G.StateConstraints([[1.0, 0.0]], [3.0], prob=0.95)    # a row that stays slack: the plan may follow the references
    H, da, x0, K, m, Tn, NO = 10, 2, pb["x0"][0], 4, 8, 5, 3
    n = H * da
    ta, tl = auglag_state_layout(K, n, H * sc.m)["total"], lbfgs_state_layout(K, n, m)["total"]
    lkw = dict(lb=-1.0, ub=1.0, history=m, gtol=1e-6, ftol=1e-12)
    log = []
    U1, c1, info1 = auglag_solve(pack, x0, X0.reshape(K, H, da), cost, sc, outer=NO, inner_ticks=Tn, check_outer=0,
                                 callback=lambda d, ws, off: log.append(ws.clone()), **lkw)
    Xd = torch.as_tensor(X0.reshape(K, H, da), device="cuda")
    al = auglag_state_new(Xd, 10.0, sc.m, lb=-1.0, ub=1.0)
    va = auglag_state_view(al, K, H, da, sc.m)
    inner = lbfgs_start(Xd, **lkw)
    vi = lbfgs_state_view(inner, K, H, da, m)
    okw = dict(lb=-1.0, ub=1.0, history=m, gtol=1e-6, ftol=1e-12, inner_ticks=Tn)
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
        for _ in range(Tn):
            r = ev()
            M, dM = auglag_merit(r["cost"], r["grad"], r["g"], r["g_jac"], va["lam"], va["rho"])
            lbfgs_tick(inner, M, dM, K, H, da, **lkw)
    vi["U"].copy_(vi["X"].view(K, H, da))
    r = ev()
    auglag_outer(al, r["cost"], r["g"], vi["U"], K, H, da, update=False, alive=vi["alive"], **okw)
    ws = log[-1]
    np.testing.assert_array_equal(_bits(al[:ta]), _bits(ws[:ta]))
    np.testing.assert_array_equal(_bits(inner[:tl]), _bits(ws[ta:ta + tl]))
    np.testing.assert_array_equal(_bits(U1), _bits(va["plan"]))
    c_plan, c_start = rc(np.asarray(U1).reshape(H, da)), rc(np.zeros((H, da)))
    print("auglag: reference cost of the plan %.6f, of the zero start %.6f" % (c_plan, c_start))
    np.testing.assert_allclose(c1, c_plan, rtol=COST_RTOL)
    assert c_plan <= c_start
    cs.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 10. refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(G):
    from gaussian_process_mpc_amd import _lib
    from gaussian_process_mpc_amd._lib import ptr, stream_ptr
    ds, da, H, B = 2, 1, 4, 3
    pb, gp, Xr, Ur, Qf = _problem(ds, da, H, B)
    pack = _pack(G, pb, gp)
    lib = G.lib()
    cs = G.CostSchedule(H, ds, da).set(Xr[:H], Ur[:H - 1], Qf)          # set for H - 1: a call of H is too long
    other = G.CostSchedule(H, ds + 1, da).set(np.zeros((H + 1, ds + 1)))
    gone = G.CostSchedule(H, ds, da).set(Xr, Ur, Qf)
    gone_id = gone.id
    gone.close()
    x0, U = torch.as_tensor(pb["x0"], device="cuda"), torch.as_tensor(pb["U"], device="cuda")
    ws = torch.empty(lib.gpmpc_rollout_workspace_bytes(pack.handle, B, H, _lib.WANT_GRAD | _lib.USE_GRAPH), dtype=torch.uint8, device="cuda")
    wsf = torch.empty(lib.gpmpc_rollout_fullcov_workspace_bytes(pack.enable_fullcov().handle, B, H, _lib.WANT_GRAD), dtype=torch.uint8, device="cuda")
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")  # noqa: E731
    cases = [("unknown", 99999, H, "cost schedule 99999 is unknown or destroyed"), ("destroyed", gone_id, H, "unknown or destroyed"),
             ("dimensions", other.id, H, "state_dim 3"), ("too long", cs.id, H, "horizon %d exceeds the horizon %d" % (H, H - 1))]
    for what, sid, Hc, text in cases:
        c = G.CostParams(-1.0, pb["Q"], pb["R"])
        c.c.schedule_id = sid
        cap = (lib.gpmpc_pack_graph_captures(pack.handle), lib.gpmpc_pack_callback_captures(pack.handle))
        for flags in (_lib.WANT_GRAD, _lib.WANT_GRAD | _lib.USE_GRAPH, 0):
            oc, og, om, ov = nan(B), nan(B, Hc, da), nan(B, Hc + 1, ds), nan(B, Hc + 1, ds)
            rc = lib.gpmpc_rollout(pack.handle, B, Hc, ptr(x0), ptr(U), ctypes.byref(c.c), flags, ptr(om), ptr(ov), ptr(oc), ptr(og),
                                   ctypes.c_void_p(ws.data_ptr()), ws.numel(), stream_ptr())
            assert rc == -1 and text in lib.gpmpc_last_error().decode(), (what, flags, rc, lib.gpmpc_last_error())
            torch.cuda.synchronize()
            assert all(bool(torch.isnan(t).all()) for t in (oc, og, om, ov)), (what, flags)
        oc, og, om, oS = nan(B), nan(B, Hc, da), nan(B, Hc + 1, ds), nan(B, Hc + 1, ds, ds)
        rc = lib.gpmpc_rollout_fullcov(pack.handle, B, Hc, ptr(x0), ptr(U), ctypes.byref(c.c), _lib.WANT_GRAD, ptr(om), ptr(oS), ptr(oc), ptr(og),
                                       ctypes.c_void_p(wsf.data_ptr()), wsf.numel(), stream_ptr())
        assert rc == -1 and text in lib.gpmpc_last_error().decode() and "gpmpc_rollout_fullcov" in lib.gpmpc_last_error().decode()
        oc, dm, dS, dU = nan(B), nan(B, Hc + 1, ds), nan(B, Hc + 1, ds, ds), nan(B, Hc, da)
        rc = lib.gpmpc_cost_grad(B, Hc, ds, da, ctypes.byref(c.c), ptr(nan(B, Hc + 1, ds)), ptr(nan(B, Hc + 1, ds, ds)), ptr(U), ptr(oc), ptr(dm),
                                 ptr(dS), ptr(dU), stream_ptr())
        assert rc == -1 and text in lib.gpmpc_last_error().decode()
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (oc, og, om, oS, dm, dS, dU)), what
        out = np.full(1 + Hc * da, np.nan)
        with pytest.raises(G.GpmpcError, match="cost schedule|exceeds the horizon"):
            pack.objective_gradient(pb["x0"][0], pb["U"][0], c)
        dp = ctypes.POINTER(ctypes.c_double)
        rc = lib.gpmpc_objective_gradient(pack.handle, Hc, pb["x0"][0].ctypes.data_as(dp), np.ascontiguousarray(pb["U"][0]).ctypes.data_as(dp),
                                          ctypes.byref(c.c), _lib.WANT_GRAD, out.ctypes.data_as(dp), stream_ptr())
        assert rc == -1 and np.all(np.isnan(out)) and text in lib.gpmpc_last_error().decode()
        assert cap == (lib.gpmpc_pack_graph_captures(pack.handle), lib.gpmpc_pack_callback_captures(pack.handle)), what
        # the constrained rollout and the three device solvers
        sc = G.StateConstraints([[1.0, 0.0]], [3.0], kappa=0.0)
        with pytest.raises(G.GpmpcError, match="cost schedule|exceeds the horizon"):
            G.rollout(pack, pb["x0"], pb["U"], c, constraints=sc)
        from gaussian_process_mpc_amd.device_auglag import auglag_solve
        from gaussian_process_mpc_amd.device_lbfgs import lbfgs_solve
        from gaussian_process_mpc_amd.mppi import mppi_solve
        with pytest.raises(G.GpmpcError, match="gpmpc_mppi_solve.*(cost schedule|exceeds the horizon)"):
            mppi_solve(pack, pb["x0"][0], np.zeros((Hc, da)), c, samples=8, iterations=1, sigma=0.5, lb=-1.0, ub=1.0)
        with pytest.raises(G.GpmpcError, match="gpmpc_lbfgs_solve.*(cost schedule|exceeds the horizon)"):
            lbfgs_solve(pack, pb["x0"][0], np.zeros((2, Hc, da)), c, lb=-1.0, ub=1.0, max_ticks=2)
        with pytest.raises(G.GpmpcError, match="gpmpc_auglag_solve.*(cost schedule|exceeds the horizon)"):
            auglag_solve(pack, pb["x0"][0], np.zeros((2, Hc, da)), c, sc, lb=-1.0, ub=1.0, outer=1, inner_ticks=1)
    # the Python object refuses a mismatch before the library is asked
    with pytest.raises(ValueError, match="dimensions"):
        G.CostParams(-1.0, pb["Q"], pb["R"], schedule=other)
    # non-finite rows: refused with a text, the schedule as it was
    good = G.CostSchedule(H, ds, da).set(Xr, Ur, Qf)
    cost = G.CostParams(-1.0, pb["Q"], pb["R"], schedule=good)
    before = G.rollout(pack, pb["x0"], pb["U"], cost, want_traj=False)
    for k, (X, Uu, Qq, text) in enumerate([(np.where(np.arange(H + 1)[:, None] == 2, np.nan, Xr), Ur, Qf, "x_ref has a non-finite"),
                                           (Xr, np.where(np.arange(H)[:, None] == 1, np.inf, Ur), Qf, "u_ref has a non-finite"),
                                           (Xr, Ur, Qf * np.where(np.eye(ds) > 0, 1.0, np.nan), "Q_terminal has a non-finite")]):
        with pytest.raises(G.GpmpcError, match=text):
            good.set(X, Uu, Qq)
    with pytest.raises(G.GpmpcError, match="outside 1..H_max"):
        good.set(np.zeros((H + 2, ds)))
    assert good.get()["H"] == H and good.get()["has_Q_terminal"]
    after = G.rollout(pack, pb["x0"], pb["U"], cost, want_traj=False)
    np.testing.assert_array_equal(_bits(before["cost"]), _bits(after["cost"]))
    np.testing.assert_array_equal(_bits(before["grad"]), _bits(after["grad"]))
    for c_ in (cs, other, good):
        c_.close()


def test_device_form_of_set_equals_the_host_form(G):
    ds, da, H, B = 2, 1, 4, 3
    pb, gp, Xr, Ur, Qf = _problem(ds, da, H, B)
    pack = _pack(G, pb, gp)
    a, b = G.CostSchedule(H, ds, da).set(Xr, Ur, Qf), G.CostSchedule(H, ds, da)
    t = lambda x: torch.as_tensor(x, device="cuda")  # noqa: E731
    b.set(t(Xr), t(Ur), t(Qf))
    ra, rb = (G.rollout(pack, pb["x0"], pb["U"], G.CostParams(-1.0, pb["Q"], pb["R"], schedule=c), want_traj=False) for c in (a, b))
    np.testing.assert_array_equal(_bits(ra["cost"]), _bits(rb["cost"]))
    np.testing.assert_array_equal(_bits(ra["grad"]), _bits(rb["grad"]))
    b.set(t(Xr), None, None)                                   # zeros for u_ref, no terminal weight -- as the host form reads NULL
    a.set(Xr, None, None)
    ra, rb = (G.rollout(pack, pb["x0"], pb["U"], G.CostParams(-1.0, pb["Q"], pb["R"], schedule=c), want_traj=False) for c in (a, b))
    np.testing.assert_array_equal(_bits(ra["cost"]), _bits(rb["cost"]))
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 11. the MPC class and the closed loop
# ------------------------------------------------------------------------------------------------------------------------------
def _mpc_c1(G):
    from oracle import gpmpc_oracle as O
    pb = _c1(G)[0]
    mpc = G.RiskSensitiveMPC(1e-5, 10, 2, 2, pb["Q"], pb["R"])
    for a, g in enumerate(mpc.dynamics.gpr_err):
        g.set_lambdas(pb["lambdas"][a])
        g.set_sigma_n(float(pb["sigma_n"][a]))
        g.set_sigma_f(1.0)
    mpc.dynamics.append_train_data(pb["X"][:, :2], pb["X"][:, 2:], pb["Y"])
    Kinv = torch.stack([g.Ky_inv.detach().cpu() for g in mpc.dynamics.gpr_err])
    gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"], Ky_inv=Kinv)
    mpc.set_lb([-1.0, -1.0])
    mpc.set_ub([1.0, 1.0])
    return mpc, gp, pb


def test_cost_torch_backward_honours_the_schedule(G):
    mpc, gp, pb = _mpc_c1(G)
    Xr, H = _c1(G)[2], 10
    Qf = T.general_weight(2, 9)
    Ur = 0.3 * np.cos(np.arange(H * 2)).reshape(H, 2)
    mpc.set_reference_trajectory(Xr, Ur, Q_terminal=Qf)
    x0, U0 = pb["x0"][0], pb["U"][0]
    ref = T.tracking_objective(gp, H, x0, U0, Xr, Ur, pb["Q"], pb["R"], 1e-5, Q_terminal=Qf)
    u = torch.as_tensor(U0, device="cuda").clone().requires_grad_(True)
    means, covs = mpc.dynamics.forward_propagate_torch(H, torch.as_tensor(x0, device="cuda"), u)
    c = mpc.cost_torch(means, u, covs, mpc.x_ref, mpc.u_ref)
    c.backward()
    np.testing.assert_allclose(c.item(), ref["cost"], rtol=COST_RTOL)
    _assert_grad(u.grad.cpu().numpy(), ref["grad"], "cost_torch backward")
    # objective / gradient / evaluate_batch read the same schedule
    mpc.curr_state = torch.as_tensor(x0, device="cuda")
    np.testing.assert_allclose(mpc.objective(U0.reshape(-1)), ref["cost"], rtol=COST_RTOL)
    _assert_grad(mpc.gradient(U0.reshape(-1)), ref["grad"], "gradient callback")
    np.testing.assert_allclose(mpc.evaluate_batch(U0[None], want_grad=False)["cost"][0].item(), ref["cost"], rtol=COST_RTOL)
    mpc.clear_reference_trajectory()                          # Q_terminal stays: the schedule repeats x_ref
    mpc.set_xref([0.2, -0.1])
    ref2 = T.tracking_objective(gp, H, x0, U0, np.tile([0.2, -0.1], (H + 1, 1)), None, pb["Q"], pb["R"], 1e-5, Q_terminal=Qf, want_grad=False)
    np.testing.assert_allclose(mpc.objective(U0.reshape(-1)), ref2["cost"], rtol=COST_RTOL)
    mpc.Q_terminal = None                                     # and without it the controller is what it was
    assert mpc._cost_params().c.schedule_id == 0


@pytest.mark.parametrize("terminal,cpu_cost", [(False, 0.038654), (True, 0.062385)])
def test_tracking_solve_against_the_cpu_solve(G, terminal, cpu_cost):
    """synth_problem(1, 100, 2, 2, 10, .) trajectory 0, gamma = 1e-5, inputs within +-1, start U = 0.  The reference trajectory is the
    predicted means under the seeded plan of trajectory 1, offset by 0.2; terminal weight 10 Q or none.  CPU figures of the same
    construction with the reference alone (scipy L-BFGS-B from the zero start, ftol 1e-10, gtol 1e-4): no terminal weight: cost of the
    zero plan 0.183634, of the solve 0.038654 (12 iterations); Q_f = 10 Q: 0.558042 -> 0.062385 (31 iterations)."""
    mpc, gp, pb = _mpc_c1(G)
    Xr, H, x0 = _c1(G)[2], 10, pb["x0"][0]
    Qf = 10.0 * pb["Q"] if terminal else None
    mpc.set_reference_trajectory(Xr, Q_terminal=Qf)
    U = mpc.get_optimal_trajectory(x0)
    assert mpc.solver_used in ("scipy-lbfgsb", "ipopt") and mpc.step_index == 1
    got = T.tracking_objective(gp, H, x0, U, Xr, None, pb["Q"], pb["R"], 1e-5, Q_terminal=Qf, want_grad=False)["cost"]
    print("tracking solve (%s): reference cost %.6f (CPU solve: %.6f, rel %.2e)" % (mpc.solver_used, got, cpu_cost, abs(got - cpu_cost) / cpu_cost))
    assert np.all(np.abs(U) <= 1.0 + 1e-9)
    np.testing.assert_allclose(got, cpu_cost, rtol=1e-3)
    # the device solvers read the same schedule: each ends below the zero plan
    zero = T.tracking_objective(gp, H, x0, np.zeros((H, 2)), Xr, None, pb["Q"], pb["R"], 1e-5, Q_terminal=Qf, want_grad=False)["cost"]
    for solver in ("mppi", "lbfgs"):
        Us = mpc.get_optimal_trajectory(x0, solver=solver, n_starts=1 if solver == "mppi" else 4)
        cs_ = T.tracking_objective(gp, H, x0, Us, Xr, None, pb["Q"], pb["R"], 1e-5, Q_terminal=Qf, want_grad=False)["cost"]
        print("  solver=%s: reference cost %.6f (zero plan %.6f)" % (solver, cs_, zero))
        assert cs_ < zero
    mpc.full_covariance = True
    assert np.isfinite(mpc.objective(np.zeros(H * 2)))


def test_sliding_reference_in_the_closed_loop(G):
    """12 pendulum steps, 100 pre-training transitions, H = 5, theta following a sinusoid through mpc.reference = fn: the window moves
    every step, the callback graph is captured once."""
    rng = np.random.default_rng(3)
    plant = G.PendulumPlant(init_state=(0.3, 0.0))
    S = np.stack((rng.uniform(-1, 1, 100), rng.uniform(-2, 2, 100)), axis=1)
    A = rng.uniform(-2, 2, (100, 1))
    nxt = np.array([G.PendulumPlant(init_state=s).step(a)[0] for s, a in zip(S, A)])
    H = 5
    mpc = G.RiskSensitiveMPC(-1.0, H, 2, 1, np.diag([10.0, 0.1]), 0.01 * np.eye(1), nominal_models=G.LinearNominalModel.identity(2, 1))
    for g in mpc.dynamics.gpr_err:
        g.set_lambdas(np.array([1.0, 4.0, 4.0]))
        g.set_sigma_n(np.array(1e-2))
    mpc.dynamics.append_train_data(S, A, nxt)
    mpc.set_lb([-2.0])
    mpc.set_ub([2.0])
    asked = []

    def window(k):
        asked.append(k)
        t = np.arange(k, k + H + 1)
        return np.stack((0.3 * np.cos(2 * np.pi * t / 24.0), np.zeros(H + 1)), axis=1)
    mpc.reference = window
    mpc.Q_terminal = np.diag([20.0, 0.2])
    hist = G.Simulator(mpc, plant, num_iters=12, incremental=True).run()
    assert asked == list(range(12)) and mpc.step_index == 12
    acts = np.array([np.asarray(h[1]).reshape(-1) for h in hist])
    assert np.all(np.isfinite(acts)) and np.all(np.abs(acts) <= 2.0 + 1e-9)
    pack = mpc.dynamics.pack()
    caps = G.lib().gpmpc_pack_callback_captures(pack.handle)
    print("closed loop: solver %s, callback captures %d, theta %s" % (mpc.solver_used, caps, np.round([h[0][0] for h in hist], 3)))
    assert mpc.solver_used in ("scipy-lbfgsb", "ipopt") and caps == 1      # both go through the callback graph of gpmpc_objective_gradient
    mpc.step_index = 40                                       # settable: the next window is the one of step 40
    mpc.get_optimal_trajectory(np.array([0.1, 0.0]))
    assert asked[-1] == 40 and mpc.step_index == 41
