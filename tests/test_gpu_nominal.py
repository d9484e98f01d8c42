"""GPU tests of the linear nominal model in the rollout: the HIP path (nominal variants of the head / tail kernels, two-launch form)
against the float64 CPU reference of tests/nominal_reference.py (pinned oracle + autograd, none of the kernels' closed forms).

Tolerances are the project's: means 1e-5, variances 1e-4, cost 1e-6 relative, directional gradients 1e-4 relative.
Inputs: synth_problem with the nominal model "identity on the states, 0.05 on every action, bias 0.01", for which the reference's
variances stay positive and 1 + gamma Q v > 0 (re-asserted on every reference trajectory used here).
"""
import ctypes

import numpy as np
import pytest
import torch

from nominal_reference import assert_reference_is_sane, nominal_rollout, synth_nominal

pytestmark = pytest.mark.gpu

MEAN_RTOL, VAR_RTOL, COST_RTOL, GRAD_RTOL = 1e-5, 1e-4, 1e-6, 1e-4
TWO_LAUNCH = ("head+pair_sb", "head+pair_sbs", "head+pair_staged")

#        tag     config N    ds da H   gamma  shared
CASES = {"c1":  (1,     100, 2, 2, 10, 1e-5,  False),
         "c2":  (2,     200, 3, 1, 20, -1.0,  False),
         "c3":  (3,     449, 4, 1, 10, -1.0,  False),
         "c3s": (3,     449, 4, 1, 10, -1.0,  True),
         "big": (3,     1024, 4, 1, 5, -1.0,  False)}
BMAX = 64
_problems, _refs = {}, {}


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    return g


def _problem(tag):
    """(pb, oracle GP bundle on the RAW targets, (W, b)) of a case, built once."""
    if tag not in _problems:
        from gaussian_process_mpc_amd.synth import synth_problem
        from oracle import gpmpc_oracle as O
        cfg, N, ds, da, H, gamma, shared = CASES[tag]
        pb = synth_problem(cfg, N, ds, da, H, BMAX, shared_lambda=shared)
        pb["gamma"] = gamma
        gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"])
        _problems[tag] = (pb, gp, synth_nominal(ds, da))
    return _problems[tag]


def _ref(tag, b):
    """Reference trajectory b of a case (cached: 0.3 ... 3 s each on the CPU)."""
    if (tag, b) not in _refs:
        pb, gp, (W, c) = _problem(tag)
        r = nominal_rollout(gp, W, c, pb["H"], pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], pb["gamma"])
        assert_reference_is_sane(r, pb["Q"], pb["gamma"])
        _refs[(tag, b)] = r
    return _refs[(tag, b)]


def _pack(G, tag, nominal="synth"):
    pb, gp, nom = _problem(tag)
    return G.GPPack(pb["X"], pb["Y"], gp.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"], nominal=nom if isinstance(nominal, str) else nominal)


def _cost(G, tag):
    pb = _problem(tag)[0]
    return G.CostParams(pb["gamma"], pb["Q"], pb["R"], x_ref=pb["x_ref"], u_ref=pb["u_ref"])


def _assert_grad(got, ref, what):
    """Directional derivatives along the reference gradient and three seeded directions, 1e-4 relative; and the whole vector in norm."""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    rng = np.random.default_rng(12345)
    dirs = [ref / np.linalg.norm(ref)] + [d / np.linalg.norm(d) for d in rng.standard_normal((3, ref.size))]
    for k, d in enumerate(dirs):
        a, e = float(got @ d), float(ref @ d)
        print("  %s: directional derivative %d: %.12g vs reference %.12g (rel %.2e)" % (what, k, a, e, abs(a - e) / abs(e)))
        assert abs(a - e) <= GRAD_RTOL * abs(e), (what, k, a, e)
    assert np.linalg.norm(got - ref) <= GRAD_RTOL * np.linalg.norm(ref), what


def _assert_traj(r, idx, ref, what, grad=True):
    m, v = r["means"][idx].cpu().numpy(), r["vars"][idx].cpu().numpy()
    print("%s: max rel mean %.2e, var %.2e, cost %.2e" % (what, np.max(np.abs(m - ref["means"]) / np.maximum(np.abs(ref["means"]), 1e-9)),
                                                         np.max(np.abs(v - ref["vars"]) / ref["vars"]),
                                                         abs(r["cost"][idx].item() - ref["cost"]) / abs(ref["cost"])))
    np.testing.assert_allclose(m, ref["means"], rtol=MEAN_RTOL, atol=1e-9)
    np.testing.assert_allclose(v, ref["vars"], rtol=VAR_RTOL, atol=1e-12)
    np.testing.assert_allclose(r["cost"][idx].item(), ref["cost"], rtol=COST_RTOL)
    if grad:
        _assert_grad(r["grad"][idx].cpu().numpy(), ref["grad"], what)


def _shapes():
    """Every (case, B, graph) the parity test runs."""
    out = [(tag, B, graph) for tag in ("c1", "c2", "c3", "c3s") for B in (1, 2, BMAX) for graph in (False, True)]
    return out + [("big", BMAX, False), ("big", BMAX, True)]


# ------------------------------------------------------------------------------------------------------------------------------
# 1. parity with the reference helper
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["c1", "c2", "c3", "c3s", "big"])
def test_parity_with_the_reference(G, tag):
    pb, gp, (W, c) = _problem(tag)
    pack, cost = _pack(G, tag), _cost(G, tag)
    got_W, got_c = pack.nominal
    np.testing.assert_array_equal(got_W, W)
    np.testing.assert_array_equal(got_c, c)
    # beta is formed from the residual targets on the device
    beta = pack.beta().cpu().numpy()
    for a in range(pb["ds"]):
        b_ref = gp.Ky_inv[a].numpy() @ (pb["Y"][:, a] - pb["X"] @ W[a] - c[a])
        np.testing.assert_allclose(beta[a], b_ref, rtol=1e-9, atol=1e-9 * np.abs(b_ref).max())
    moved = 0.0
    for (t, B, graph) in _shapes():
        if t != tag:
            continue
        plan = pack.plan(B, pb["H"], want_grad=True, graph=graph)
        assert plan["form"] in TWO_LAUNCH and plan.get("nominal") == 1 and plan["hchunks"] == 0, plan
        if B == BMAX and tag in ("c3", "c3s", "big"):
            assert plan["form"] == ("head+pair_sbs" if tag == "c3s" else "head+pair_sb"), plan
        r = G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=True, graph=graph)
        torch.cuda.synchronize()
        for b in sorted({0, B - 1}):
            _assert_traj(r, b, _ref(tag, b), "%s B=%d graph=%s [%d] %s" % (tag, B, graph, b, plan["form"]))
        ro = G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=False, graph=graph)      # objective only: the <D, 1> head instances
        torch.cuda.synchronize()
        for b in sorted({0, B - 1}):
            _assert_traj(ro, b, _ref(tag, b), "%s B=%d graph=%s [%d] objective only" % (tag, B, graph, b), grad=False)
    # the solver callback (host in, host out, captured graph)
    for b in (0, BMAX - 1):
        ref = _ref(tag, b)
        cg = pack.objective_gradient(pb["x0"][b], pb["U"][b], cost)
        np.testing.assert_allclose(cg[0], ref["cost"], rtol=COST_RTOL)
        _assert_grad(cg[1:], ref["grad"], "%s callback [%d]" % (tag, b))
        c_only = pack.objective_gradient(pb["x0"][b], pb["U"][b], cost, want_grad=False)
        np.testing.assert_allclose(c_only[0], ref["cost"], rtol=COST_RTOL)
    # ... and none of this could pass on a rollout that ignores the model: it moves the means by orders of magnitude more than the tolerance
    from oracle import gpmpc_oracle as O
    plain = O.objective_and_gradient(gp, pb["H"], pb["x0"][0], pb["U"][0], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], pb["gamma"], mode="o2")
    moved = np.max(np.abs(plain["means"][1:] - _ref(tag, 0)["means"][1:]))
    print("%s: the nominal model moves the means by up to %.3g" % (tag, moved))
    assert moved > 1e-3


def test_every_two_launch_form_and_a_split_are_reached(G):
    """The shapes of the parity test, by their plans: scalar-broadcast, shared-lambda and staged pair kernels and concurrent
    sub-batches are each reached, always as a nominal plan."""
    forms, splits, tilings = set(), set(), set()
    packs = {}
    for (tag, B, graph) in _shapes():
        if tag not in packs:
            packs[tag] = _pack(G, tag)
        plan = packs[tag].plan(B, CASES[tag][4], want_grad=True, graph=graph)
        assert plan.get("nominal") == 1 and plan["launches_per_step"] == 2, plan
        forms.add(plan["form"])
        splits.add(plan["split"])
        tilings.add((plan["form"], plan["tiling"]))
    print(sorted(forms), sorted(splits), sorted(tilings))
    assert forms == set(TWO_LAUNCH), forms
    assert max(splits) > 1, splits
    # a pack without the model plans the same shapes differently (one launch per step, or the whole horizon): no "nominal" field
    pb, gp, _ = _problem("c3")
    plain = G.GPPack(pb["X"], pb["Y"], gp.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"])
    p1 = plain.plan(1, pb["H"])
    assert "nominal" not in p1 and p1["launches_per_step"] != 2, p1
    assert plain.nominal is None


def test_parity_on_the_staged_pair_kernel_when_forced(G, monkeypatch):
    """GPMPC_PAIR_SB=0: a batch that would run the scalar-broadcast kernel goes through head + staged pair_kernel.h."""
    pb = _problem("c3")[0]
    pack, cost = _pack(G, "c3"), _cost(G, "c3")
    assert pack.plan(BMAX, pb["H"])["form"] == "head+pair_sb"
    monkeypatch.setenv("GPMPC_PAIR_SB", "0")
    pack.reload_tuning()
    try:
        plan = pack.plan(BMAX, pb["H"])
        assert plan["form"] == "head+pair_staged" and plan.get("nominal") == 1, plan
        r = G.rollout(pack, pb["x0"], pb["U"], cost, want_grad=True)
        torch.cuda.synchronize()
        for b in (0, BMAX - 1):
            _assert_traj(r, b, _ref("c3", b), "c3 staged forced [%d]" % b)
    finally:
        monkeypatch.delenv("GPMPC_PAIR_SB")
        pack.reload_tuning()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. zero coefficients == the plain pack in the two-launch form
# ------------------------------------------------------------------------------------------------------------------------------
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
    return means.cpu().numpy(), vars_.cpu().numpy(), jac.cpu().numpy()


def _close12(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    scale = np.max(np.abs(b))
    print("  %s: max abs difference %.3e at scale %.3e" % (what, np.max(np.abs(a - b)), scale))
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12 * scale, err_msg=what)


@pytest.mark.parametrize("tag", ["c1", "c3", "c3s"])
def test_zero_coefficients_equal_the_plain_two_launch_rollout(G, tag, monkeypatch):
    pb, gp, _ = _problem(tag)
    cost = _cost(G, tag)
    zero = (np.zeros((pb["ds"], pb["ds"] + pb["da"])), np.zeros(pb["ds"]))
    nom = _pack(G, tag, nominal=zero)
    for k in ("GPMPC_FUSED", "GPMPC_FUSED_SB", "GPMPC_PERSIST"):
        monkeypatch.setenv(k, "0")
    plain = G.GPPack(pb["X"], pb["Y"], gp.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"])          # (overrides are read at pack creation)
    for k in ("GPMPC_FUSED", "GPMPC_FUSED_SB", "GPMPC_PERSIST"):
        monkeypatch.delenv(k)
    for B in (1, 2, BMAX):
        pn, pp = nom.plan(B, pb["H"]), plain.plan(B, pb["H"])
        assert pn["form"] == pp["form"] and pn["tiling"] == pp["tiling"] and pn["split"] == pp["split"], (pn, pp)
        assert pn.get("nominal") == 1 and "nominal" not in pp
        a = G.rollout(nom, pb["x0"][:B], pb["U"][:B], cost, want_grad=True)
        b = G.rollout(plain, pb["x0"][:B], pb["U"][:B], cost, want_grad=True)
        torch.cuda.synchronize()
        for key in ("means", "vars", "cost", "grad"):
            _close12(a[key].cpu().numpy(), b[key].cpu().numpy(), "%s B=%d %s" % (tag, B, key))
        ja, jb = _rollout_jac(nom, pb["x0"][:B], pb["U"][:B]), _rollout_jac(plain, pb["x0"][:B], pb["U"][:B])
        for name, x, y in zip(("jac means", "jac vars", "jacobians"), ja, jb):
            _close12(x, y, "%s B=%d %s" % (tag, B, name))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. known answer: exactly linear targets
# ------------------------------------------------------------------------------------------------------------------------------
def test_linear_targets_give_the_linear_recursion(G):
    from oracle import gpmpc_oracle as O
    pb, gp0, (W, c) = _problem("c3")
    ds, H = pb["ds"], pb["H"]
    Y = pb["X"] @ W.T + c                                                   # beta = Ky_inv (Y - X W^T - c) = 0
    gp = O.GPBundle(pb["X"], Y, pb["lambdas"], pb["sigma_f"], pb["sigma_n"], Ky_inv=gp0.Ky_inv)
    pack = G.GPPack(pb["X"], Y, gp0.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"], nominal=(W, c))
    assert np.max(np.abs(pack.beta().cpu().numpy())) < 1e-8
    B = 4
    r = G.rollout(pack, pb["x0"][:B], pb["U"][:B], _cost(G, "c3"), want_grad=True)
    torch.cuda.synchronize()
    for b in range(B):
        lin = [pb["x0"][b]]
        for t in range(H):
            lin.append(W[:, :ds] @ lin[-1] + W[:, ds:] @ pb["U"][b, t] + c)
        np.testing.assert_allclose(r["means"][b].cpu().numpy(), np.array(lin), rtol=MEAN_RTOL, atol=1e-9)
        ref = nominal_rollout(gp, W, c, H, pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], pb["gamma"])
        assert_reference_is_sane(ref, pb["Q"], pb["gamma"])
        np.testing.assert_allclose(ref["means"], np.array(lin), rtol=1e-9, atol=1e-9)
        _assert_traj(r, b, ref, "linear targets [%d]" % b)                 # variances: v_g(beta = 0) + sum_k n_k^2 s_k, from the helper


# ------------------------------------------------------------------------------------------------------------------------------
# 4. autograd through Dynamics / RiskSensitiveMPC
# ------------------------------------------------------------------------------------------------------------------------------
def _mpc_identity(G, tag):
    from oracle import gpmpc_oracle as O
    pb = _problem(tag)[0]
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    mpc = G.RiskSensitiveMPC(pb["gamma"], H, ds, da, pb["Q"], pb["R"], nominal_models=G.LinearNominalModel.identity(ds, da))
    for a, g in enumerate(mpc.dynamics.gpr_err):
        g.set_lambdas(pb["lambdas"][a])
        g.set_sigma_n(float(pb["sigma_n"][a]))
        g.set_sigma_f(1.0)
    mpc.dynamics.append_train_data(pb["X"][:, :ds], pb["X"][:, ds:], pb["Y"])
    Kinv = torch.stack([g.Ky_inv.detach().cpu() for g in mpc.dynamics.gpr_err])
    gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"], Ky_inv=Kinv)
    W = np.concatenate((np.eye(ds), np.zeros((ds, da))), axis=1)
    return mpc, gp, W, np.zeros(ds)


@pytest.mark.parametrize("tag", ["c1", "c2"])
def test_autograd_through_dynamics_with_identity_nominal(G, tag):
    pb = _problem(tag)[0]
    H, da = pb["H"], pb["da"]
    mpc, gp, W, c = _mpc_identity(G, tag)
    pack = mpc.dynamics.pack()
    got_W, got_c = pack.nominal
    np.testing.assert_array_equal(got_W, W)
    np.testing.assert_array_equal(got_c, c)
    # the GPs learn the state difference
    for a, g in enumerate(mpc.dynamics.gpr_err):
        np.testing.assert_allclose(g.beta().cpu().numpy(), (gp.Ky_inv[a] @ (gp.Y[:, a] - gp.X[:, a])).numpy(), rtol=1e-8, atol=1e-8)
    for b in (0, 1):
        ref = nominal_rollout(gp, W, c, H, pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], pb["gamma"], want_x0_grad=True)
        assert_reference_is_sane(ref, pb["Q"], pb["gamma"])
        x0 = torch.tensor(pb["x0"][b], dtype=torch.float64, device=mpc.device).requires_grad_(True)
        u = torch.tensor(pb["U"][b], dtype=torch.float64, device=mpc.device).requires_grad_(True)
        means, covs = mpc.dynamics.forward_propagate_torch(H, x0, u)
        np.testing.assert_allclose(torch.stack(means).detach().cpu().numpy(), ref["means"], rtol=MEAN_RTOL, atol=1e-9)
        np.testing.assert_allclose(torch.stack([s.diagonal() for s in covs]).detach().cpu().numpy(), ref["vars"], rtol=VAR_RTOL, atol=1e-12)
        cost = mpc.cost_torch(means, u, covs, mpc.x_ref, mpc.u_ref)
        cost.backward()
        np.testing.assert_allclose(cost.item(), ref["cost"], rtol=COST_RTOL)
        _assert_grad(u.grad.cpu().numpy(), ref["grad"], "%s autograd dU [%d]" % (tag, b))
        _assert_grad(x0.grad.cpu().numpy(), ref["grad_x0"], "%s autograd dx0 (gpmpc_rollout_vjp) [%d]" % (tag, b))
        # the solver callbacks of the same object, the numpy rollout and the batched rollout
        mpc.curr_state = torch.tensor(pb["x0"][b], dtype=torch.float64, device=mpc.device)
        mpc._cache_key = None
        x = pb["U"][b].reshape(-1).copy()
        np.testing.assert_allclose(mpc.objective(x), ref["cost"], rtol=COST_RTOL)
        _assert_grad(mpc.gradient(x), ref["grad"], "%s callbacks [%d]" % (tag, b))
        m_np, c_np = mpc.dynamics.forward_propagate(H, pb["x0"][b], pb["U"][b])
        np.testing.assert_allclose(m_np, ref["means"], rtol=MEAN_RTOL, atol=1e-9)
        np.testing.assert_allclose(np.array([np.diag(s) for s in c_np]), ref["vars"], rtol=VAR_RTOL, atol=1e-12)
    r = mpc.dynamics.rollout(pb["x0"][:2], pb["U"][:2], cost=mpc._cost_params(), want_grad=True)
    _assert_grad(r["grad"][1].cpu().numpy(), ref["grad"], "%s Dynamics.rollout [1]" % tag)
    with pytest.raises(NotImplementedError):
        mpc.dynamics.rollout(pb["x0"][:2], pb["U"][:2], full_covariance=True)


def test_multistart_solve_with_nominal_models(G):
    """n_starts = K: every tick is one batched graph rollout of the nominal pack; the result is no worse than the zero plan."""
    pb = _problem("c1")[0]
    mpc, gp, W, c = _mpc_identity(G, "c1")
    mpc.set_lb([-1.0] * pb["da"]); mpc.set_ub([1.0] * pb["da"])
    mpc.multistart_options["max_ticks"] = 15
    U = mpc.get_optimal_trajectory(pb["x0"][0], n_starts=4)
    assert U.shape == (pb["H"], pb["da"]) and np.all(np.isfinite(U)) and np.all(np.abs(U) <= 1.0 + 1e-9)
    assert mpc.dynamics.pack().plan(16, pb["H"], graph=True).get("nominal") == 1
    ref = nominal_rollout(gp, W, c, pb["H"], pb["x0"][0], U, pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], pb["gamma"], want_grad=False)
    ref0 = nominal_rollout(gp, W, c, pb["H"], pb["x0"][0], np.zeros_like(U), pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], pb["gamma"], want_grad=False)
    assert ref["cost"] <= ref0["cost"] + 1e-9, (ref["cost"], ref0["cost"])


# ------------------------------------------------------------------------------------------------------------------------------
# 5. lifecycle
# ------------------------------------------------------------------------------------------------------------------------------
def test_lifecycle_of_the_nominal_model(G):
    from gaussian_process_mpc_amd import _lib
    from gaussian_process_mpc_amd._lib import lib, host_doubles, stream_ptr, ptr, GpmpcError
    from gaussian_process_mpc_amd.synth import synth_problem
    from oracle import gpmpc_oracle as O
    ds, da, H = 4, 1, 6
    pb = synth_problem(3, 470, ds, da, H, 4)
    W, c = synth_nominal(ds, da)
    n1 = 449                                                                 # 449 and 470 share the padded size 512
    gp1 = O.GPBundle(pb["X"][:n1], pb["Y"][:n1], pb["lambdas"], pb["sigma_f"], pb["sigma_n"])
    gp2 = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"])
    cost = G.CostParams(-1.0, pb["Q"], pb["R"])
    pack = G.GPPack(pb["X"][:n1], pb["Y"][:n1], gp1.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"], nominal=(W, c))
    h = pack.handle

    def ref_of(gp, b=0):
        r = nominal_rollout(gp, W, c, H, pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], -1.0)
        assert_reference_is_sane(r, pb["Q"], -1.0)
        return r

    cg = pack.objective_gradient(pb["x0"][0], pb["U"][0], cost)
    np.testing.assert_allclose(cg[0], ref_of(gp1)["cost"], rtol=COST_RTOL)
    cap0 = lib().gpmpc_pack_callback_captures(h)
    assert cap0 >= 1
    # -- argument errors: exactly one of the two pointers
    assert lib().gpmpc_pack_set_nominal(h, host_doubles(W)[1], None, stream_ptr()) == -1
    assert lib().gpmpc_pack_set_nominal(h, None, host_doubles(c)[1], stream_ptr()) == -1
    np.testing.assert_array_equal(pack.nominal[0], W)                        # ... and nothing changed
    G.rollout(pack, pb["x0"], pb["U"], cost)
    # -- resize + build keep the coefficients (GPPack.rebuild: gpmpc_pack_resize, then the build from raw targets)
    assert pack.rebuild(pb["X"], pb["Y"], gp2.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"])
    assert pack.handle is h and pack.N == 470
    np.testing.assert_array_equal(pack.nominal[0], W)
    np.testing.assert_array_equal(pack.nominal[1], c)
    r = G.rollout(pack, pb["x0"], pb["U"], cost)
    torch.cuda.synchronize()
    _assert_traj(r, 0, ref_of(gp2), "after resize + build")
    cg = pack.objective_gradient(pb["x0"][0], pb["U"][0], cost)
    np.testing.assert_allclose(cg[0], ref_of(gp2)["cost"], rtol=COST_RTOL)
    assert lib().gpmpc_pack_callback_captures(h) == cap0                     # the refill replays the captured callback graph
    # -- new coefficients: "not built" until the next build
    W2 = W.copy(); W2[:, ds:] = 0.1
    assert lib().gpmpc_pack_set_nominal(h, host_doubles(W2)[1], host_doubles(c)[1], stream_ptr()) == 0
    with pytest.raises(GpmpcError, match="not built"):
        G.rollout(pack, pb["x0"], pb["U"], cost)
    with pytest.raises(GpmpcError, match="not built"):
        pack.objective_gradient(pb["x0"][0], pb["U"][0], cost)
    assert lib().gpmpc_pack_shared_lambda(h) == -5
    np.testing.assert_array_equal(pack.nominal[0], W2)
    assert pack.rebuild(pb["X"], pb["Y"], gp2.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"], nominal=(W, c))     # back to (W, c)
    r = G.rollout(pack, pb["x0"], pb["U"], cost)
    torch.cuda.synchronize()
    _assert_traj(r, 1, ref_of(gp2, 1), "after set_nominal + build")
    assert lib().gpmpc_pack_callback_captures(h) == cap0                     # new VALUES of a model that stays on: no re-capture
    # -- entry points that cannot honour the model refuse, and say why
    with pytest.raises(NotImplementedError):
        G.rollout_fullcov(pack, pb["x0"], pb["U"], cost)
    with pytest.raises(NotImplementedError):
        G.moment_match(pack, np.zeros(ds + da), 1e-3 * np.eye(ds + da))
    for prec in ("fp32acc", "fp32"):
        with pytest.raises(GpmpcError, match="nominal model"):
            G.rollout(pack, pb["x0"], pb["U"], cost, want_grad=False, precision=prec)
    assert lib().gpmpc_moment_match(h, 1, *([None] * 2), 0, *([None] * 10), None, 0, None) == -5
    assert b"nominal model" in lib().gpmpc_last_error()
    B = 2
    e = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=pack.device)  # noqa: E731
    x0d, Ud, md, cd, od, ws = e(B, ds), e(B, H, da), e(B, H + 1, ds), e(B, H + 1, ds, ds), e(B), e(1024)
    rc = lib().gpmpc_rollout_fullcov(h, B, H, ptr(x0d), ptr(Ud), ctypes.byref(cost.c), 0, ptr(md), ptr(cd), ptr(od), None,
                                     ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr())
    assert rc == -5 and b"gpmpc_rollout_fullcov" in lib().gpmpc_last_error()
    # -- clearing returns to the default plan and drops the captured graphs
    assert pack.plan(1, H).get("nominal") == 1 and pack.plan(1, H)["launches_per_step"] == 2
    assert pack.rebuild(pb["X"], pb["Y"], gp2.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"], nominal=None)
    assert pack.nominal is None and lib().gpmpc_pack_get_nominal(h, None, None) == 0
    p1 = pack.plan(1, H)
    assert "nominal" not in p1 and (p1["form"].startswith("fused") or p1["form"] == "persist"), p1
    plain = O.objective_and_gradient(gp2, H, pb["x0"][0], pb["U"][0], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], -1.0, mode="o2")
    cg = pack.objective_gradient(pb["x0"][0], pb["U"][0], cost)
    np.testing.assert_allclose(cg[0], plain["cost"], rtol=COST_RTOL)
    np.testing.assert_allclose(cg[1:].reshape(H, da), plain["grad"], rtol=1e-4, atol=1e-7)
    assert lib().gpmpc_pack_callback_captures(h) > cap0
    r = G.rollout(pack, pb["x0"], pb["U"], cost, graph=True)
    np.testing.assert_allclose(r["cost"][0].item(), plain["cost"], rtol=COST_RTOL)
    assert _lib.WANT_GRAD == 1


# ------------------------------------------------------------------------------------------------------------------------------
# 6. closed loop
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_train", [None, 40])
def test_closed_loop_with_identity_nominal(G, max_train):
    from gaussian_process_mpc_amd._lib import lib
    rng = np.random.default_rng(3)
    plant = G.PendulumPlant(init_state=(0.3, 0.0))
    S = np.stack((rng.uniform(-1, 1, 40), rng.uniform(-2, 2, 40)), axis=1)
    A = rng.uniform(-2, 2, (40, 1))
    nxt = np.array([G.PendulumPlant(init_state=s).step(a)[0] for s, a in zip(S, A)])
    mpc = G.RiskSensitiveMPC(-1.0, 5, 2, 1, 0.5 * np.eye(2), 0.01 * np.eye(1), nominal_models=G.LinearNominalModel.identity(2, 1))
    for g in mpc.dynamics.gpr_err:
        g.set_lambdas(np.array([1.0, 4.0, 4.0]))
        g.set_sigma_n(np.array(1e-2))
    mpc.dynamics.append_train_data(S, A, nxt)
    mpc.set_lb([-2.0]); mpc.set_ub([2.0])
    p0 = mpc.dynamics.pack()
    h0 = p0.handle
    assert p0.nominal is not None and p0.plan(1, 5).get("nominal") == 1
    steps = 20                                                                # 40 + 20 points stay within the padded size 64
    sim = G.Simulator(mpc, plant, num_iters=steps, incremental=True, max_train=max_train)
    hist = sim.run()
    assert len(hist) == steps and all(np.isfinite(h[2]) for h in hist) and all(abs(h[1][0]) <= 2.0 + 1e-9 for h in hist)
    p1 = mpc.dynamics.pack()
    assert p1 is p0 and p1.handle is h0                                       # refilled, not recreated
    assert p1.N == (40 if max_train else 40 + steps)
    np.testing.assert_array_equal(p1.nominal[0], np.eye(3)[:2])
    assert lib().gpmpc_pack_callback_captures(h0) == 1                        # one capture of the callback graph for the whole loop
    # the model the loop ended with, against the reference on the same training set
    from oracle import gpmpc_oracle as O
    dyn = mpc.dynamics
    Xn, Yn = dyn.gpr_err[0].X_train.cpu().numpy(), np.stack([g.y_train.cpu().numpy().reshape(-1) for g in dyn.gpr_err], axis=1)
    Kinv = torch.stack([g.Ky_inv.detach().cpu() for g in dyn.gpr_err])
    gp = O.GPBundle(Xn, Yn, np.tile([1.0, 4.0, 4.0], (2, 1)), np.ones(2), np.full(2, 1e-2), Ky_inv=Kinv)
    U = 0.5 * np.ones((5, 1))
    ref = nominal_rollout(gp, np.eye(3)[:2], np.zeros(2), 5, hist[-1][0], U, np.zeros(2), np.zeros(1), 0.5 * np.eye(2), 0.01 * np.eye(1), -1.0)
    assert_reference_is_sane(ref, 0.5 * np.eye(2), -1.0)
    mpc.curr_state = torch.tensor(hist[-1][0], dtype=torch.float64, device=mpc.device)
    mpc._cache_key = None
    np.testing.assert_allclose(mpc.objective(U.reshape(-1)), ref["cost"], rtol=COST_RTOL)
    _assert_grad(mpc.gradient(U.reshape(-1)), ref["grad"], "closed loop, last model")
