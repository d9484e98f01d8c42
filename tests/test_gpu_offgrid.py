"""Every rollout kernel form OFF the grid the other GPU tests sit on: per-GP amplitudes sigma_f in [0.6, 1.8] (distinct), non-zero x_ref / u_ref,
a coupled Q (tests/offgrid_problems.py).  Each form has its own amplitude code -- pack_build.hip folds sf^4 into the pair weights, step.hip forms
sf^2 / sqrt(det) and var = sf^2 - T - mu^2 (and again in its nominal twin), step_fused.h, traj_persist.h and fullcov.hip keep their own copies, the
cross-unit weights carry sf_a^2 sf_b^2, the shared-lambda forms share one exponent over a group of GPs but not one amplitude -- and every one of
those factors is 1 in the other rollout tests.

References: the plain-C ports (pinned to the torch oracle ON THESE INPUTS by tests/test_host_offgrid.py, which also shows that a result with the
amplitudes dropped or permuted misses the tolerances below by a factor of 100 and more), tests/nominal_reference.py for packs with a nominal
model, tests/constraints_reference.py for Jacobians.  Every reference trajectory is re-asserted sane (variances > 0, 1 + gamma diag(Q) var > 0,
covariances positive definite) where it is computed, once per module.

Tolerances are the project's: means 1e-5 (atol 1e-9), variances / covariances 1e-4, cost 1e-6, gradient 1e-4 (directional derivatives and
norm, as tests/test_gpu_nominal.py).  Each case asserts from the plan that the intended form ran.

Observed on an MI355X, worst deviation per form as a fraction of its tolerance (means | variances or covariances | cost | gradient in norm):
    fused_staged 1e-5 | 3e-4 | 1e-4 | 2e-6        fused_sb 64 / 32 / 16 columns 5e-5 | 3e-4 | 4e-4 | 1e-6        balanced runs 3e-5 | 3e-3 | 1e-4 | 5e-6
    head+pair_sb 256x64 / 256x256 7e-6 | 6e-4 | 4e-4 | 3e-6        256x128 4e-4 | 1.2e-2 | 7e-4 | 1e-5        head+pair_staged 5e-5 | 2e-4 | 7e-4 | 1e-6
    persist 9e-6 | 6e-4 | 3e-4 | 1e-6        one lambda (pair_sbs, fused_sb_shared, persist over units) 4e-3 | 4e-3 | 4e-4 | 4e-6
    full covariance two- / four-launch 3e-5 | 1.4e-2 | 3e-4 | 1e-5        cross-unit kernel 1e-5 | 9e-5 | 4e-6 | 1e-6        nominal 2e-4 | 3e-3 | 2e-4 | 1e-5
    constraints 8e-4, dense Jacobian 4e-5        moment_match 1e-5 | 3e-5        class path 4e-4 | 1e-3 | 1e-4 | 2e-6
    action_dim >= 3 (section 8): staged 64x64 2e-5 | 2.2e-3 | 7e-4 | 6e-6        256x256 3e-5 | 7e-4 | 2e-4 | 4e-6        64x128 behind row chunks 5e-6 | 3e-4 | 2e-5 | 2e-6
    its full covariance (four-launch) 4e-6 | 2e-4 | 4e-5 | 1e-6        nominal 1e-6 | 2e-4 | 1e-4 | 1e-6        noise model 2e-5 | 2e-5 | 5e-5 | 1e-6
    constraints 1e-4, dense Jacobian rows 3e-9 relative        autograd path against the fused adjoint: equal        inert overrides: bit-equal
No form deviates by more than 1.4 % of a tolerance: no kernel was found wrong.
(What these fractions mean in units of rounding error, form by form: tests/test_gpu_accuracy.py.  The step tables live in tests/offgrid_problems.py.)
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import offgrid_problems as OG
from constraints_reference import reference_constraints
from nominal_reference import assert_reference_is_sane, nominal_rollout, synth_nominal

pytestmark = pytest.mark.gpu

MEAN_RTOL, VAR_RTOL, COST_RTOL, GRAD_RTOL = OG.GPU_MEAN_RTOL, OG.GPU_VAR_RTOL, OG.GPU_COST_RTOL, OG.GPU_GRAD_RTOL
NO_PERSIST = OG.NO_PERSIST
_refs = {}


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


def _pack(G, pb, kinv, **kw):
    return G.GPPack(pb["X"], pb["Y"], kinv, pb["lambdas"], pb["sigma_f"], **kw)


def _cost(G, pb, gamma=-1.0, **kw):
    return G.CostParams(gamma, pb["Q"], pb["R"], x_ref=pb["x_ref"], u_ref=pb["u_ref"], **kw)


def _np(r):
    return {k: v.detach().cpu().numpy().copy() for k, v in r.items()}


def _ref_diag(args, gamma, pick):
    """C-port trajectories ``pick`` of a problem: computed once per module, sanity re-asserted."""
    from oracle import cport
    pb, kinv = OG.problem(*args)
    miss = [b for b in pick if ("d", args, gamma, b) not in _refs]
    if miss:
        c = cport.rollout(pb, kinv, gamma, x0=pb["x0"][miss], U=pb["U"][miss], nthreads=8)
        OG.assert_diag_reference_is_sane(c["means"], c["vars"], c["cost"], pb["Q"], gamma)
        for k, b in enumerate(miss):
            _refs[("d", args, gamma, b)] = {key: c[key][k] for key in c}
    return {key: np.stack([_refs[("d", args, gamma, b)][key] for b in pick]) for key in ("means", "vars", "cost", "grad")}


def _ref_fullcov(args, pick):
    """Full-covariance C-port trajectories with two seeded directions each (complex-step directional derivatives)."""
    from oracle import cport
    pb, kinv = OG.problem(*args)
    H, da = pb["H"], pb["da"]
    dirs = {b: np.random.default_rng(1000 + b).normal(size=(2, H, da)) for b in pick}
    miss = [b for b in pick if ("f", args, b) not in _refs]
    if miss:
        c = cport.rollout_fullcov(pb, kinv, -1.0, x0=pb["x0"][miss], U=pb["U"][miss], dirs=np.stack([dirs[b] for b in miss]), nthreads=8)
        OG.assert_fullcov_reference_is_sane(c["means"], c["covs"], c["cost"])
        for k, b in enumerate(miss):
            _refs[("f", args, b)] = {key: c[key][k] for key in c}
    out = {key: np.stack([_refs[("f", args, b)][key] for b in pick]) for key in ("means", "covs", "cost", "ddir")}
    out["dirs"] = np.stack([dirs[b] for b in pick])
    return out


def _excess(a, b, rtol, atol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (atol + rtol * np.abs(b))))


def _assert_grad(got, ref, what):
    """The project's gradient criterion (tests/test_gpu_nominal.py::_assert_grad): directional derivatives along the reference gradient and three
    seeded directions, 1e-4 relative; and the whole vector in norm.  Returns the relative error in norm."""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    rng = np.random.default_rng(12345)
    dirs = [ref / np.linalg.norm(ref)] + [d / np.linalg.norm(d) for d in rng.standard_normal((3, ref.size))]
    for k, d in enumerate(dirs):
        a, e = float(got @ d), float(ref @ d)
        assert abs(a - e) <= GRAD_RTOL * abs(e), (what, k, a, e)
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    assert err <= GRAD_RTOL, (what, err)
    return err


def _check_diag(r, ref, pick, what, grad=True):
    """Trajectories ``pick`` of a rollout result against the reference; prints the deviations as fractions of the tolerances before it asserts."""
    r = r if isinstance(r["cost"], np.ndarray) else _np(r)
    assert all(np.all(np.isfinite(v)) for v in r.values()), what
    m, v, c = r["means"][pick], r["vars"][pick], r["cost"][pick]
    gerr = max(np.linalg.norm(r["grad"][b] - ref["grad"][k]) / np.linalg.norm(ref["grad"][k]) for k, b in enumerate(pick)) if grad else 0.0
    print("DEV %s: means %.3g vars %.3g cost %.3g grad %.3g of the tolerance" % (
        what, _excess(m, ref["means"], MEAN_RTOL, 1e-9), _excess(v, ref["vars"], VAR_RTOL, 1e-12), _excess(c, ref["cost"], COST_RTOL, 0.0), gerr / GRAD_RTOL))
    np.testing.assert_allclose(m, ref["means"], rtol=MEAN_RTOL, atol=1e-9, err_msg=what)
    np.testing.assert_allclose(v, ref["vars"], rtol=VAR_RTOL, atol=1e-12, err_msg=what)
    np.testing.assert_allclose(c, ref["cost"], rtol=COST_RTOL, err_msg=what)
    if grad:
        for k, b in enumerate(pick):
            _assert_grad(r["grad"][b], ref["grad"][k], "%s [%d]" % (what, b))


def _check_fullcov(r, ref, pick, what, grad=True):
    r = _np(r)
    assert all(np.all(np.isfinite(v)) for v in r.values()), what
    scale = np.abs(ref["covs"]).max()
    dd = np.array([[float((r["grad"][b] * ref["dirs"][k, d]).sum()) for d in range(2)] for k, b in enumerate(pick)]) if grad else ref["ddir"]
    print("DEV %s: means %.3g covs %.3g cost %.3g ddir %.3g of the tolerance" % (
        what, _excess(r["means"][pick], ref["means"], MEAN_RTOL, 1e-9), _excess(r["covs"][pick], ref["covs"], VAR_RTOL, 1e-6 * scale),
        _excess(r["cost"][pick], ref["cost"], COST_RTOL, 0.0), _excess(dd, ref["ddir"], GRAD_RTOL, 1e-7)))
    np.testing.assert_allclose(r["means"][pick], ref["means"], rtol=MEAN_RTOL, atol=1e-9, err_msg=what)
    np.testing.assert_allclose(r["covs"][pick], ref["covs"], rtol=VAR_RTOL, atol=1e-6 * scale, err_msg=what)
    np.testing.assert_allclose(r["cost"][pick], ref["cost"], rtol=COST_RTOL, err_msg=what)
    np.testing.assert_allclose(dd, ref["ddir"], rtol=GRAD_RTOL, atol=1e-7, err_msg=what)


def _run_diag(G, pack, pb, cost, B, args, gamma, what, graph=False):
    """Objective + gradient and objective only of the first B trajectories, both against the reference."""
    pick = OG.picks(B)
    ref = _ref_diag(args, gamma, pick)
    r = _np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, graph=graph))
    f = _np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=False, graph=graph))       # the GRAD = false instances
    _check_diag(r, ref, pick, what)
    _check_diag(f, ref, pick, what + " objective only", grad=False)
    return r


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the diagonal form ladder
# ------------------------------------------------------------------------------------------------------------------------------
LADDER_EXPECTED = OG.LADDER_EXPECTED


@pytest.mark.parametrize("ds,da", OG.LADDER_DIMS)
def test_diag_form_ladder_vs_cport(G, ds, da):
    """tests/test_gpu_instances.py::test_diag_rollout_every_shape_vs_cport off the grid (N = 150, H = 3: one row tile, three column chunks), each
    form forced where the default plan would take another and asserted from the plan; objective + gradient and objective only; one captured
    graph per dimension.  (ds = 1 has no GP index to confuse; the ladder costs nothing there, so it runs whole.)"""
    D = ds + da
    bs = OG.ladder_batches(ds)
    args = (OG.ladder_config(ds, da), OG.LADDER_N, ds, da, OG.LADDER_H, bs["big"], False)
    pb, kinv = OG.problem(*args)
    H = pb["H"]
    pack, cost = _pack(G, pb, kinv), _cost(G, pb)
    steps = OG.ladder_steps(ds)                              # (B, overrides, form, tiling, tag, how the kernel name shows it)
    reached = set()
    for B, env, form, tiling, tag, kern in steps:
        with _tuning(pack, env):
            plan = pack.plan(B, H)
            OG.assert_ladder_plan(plan, (B, env, form, tiling, tag, kern), D)
            assert pack.plan(B, H, want_grad=False)["form"] == form
            _run_diag(G, pack, pb, cost, B, args, -1.0, "ds=%d da=%d B=%d %s %s %s" % (ds, da, B, form, tiling, tag))
            if tag == "tb1":                          # the captured graph of this dimension: head + pair kernel in concurrent sub-batches
                gplan = pack.plan(B, H, graph=True)
                assert gplan["form"] == form and gplan["tiling"] == tiling, gplan
                _run_diag(G, pack, pb, cost, B, args, -1.0, "ds=%d da=%d B=%d %s %s graph split=%d" % (ds, da, B, form, tiling, gplan["split"]), graph=True)
        reached.add((form, tiling, tag))
    print(sorted(reached))
    assert reached == LADDER_EXPECTED, reached ^ LADDER_EXPECTED


@pytest.mark.parametrize("tag", ["256x128", "runs"])
def test_wide_tilings_vs_cport(G, tag):
    """The two tilings a training set of one row tile cannot reach.
    256x128 tiles, two trajectories per wave (plan.hip: only for Np > 512): N = 520 pads to 576, the smallest padded size beyond 512; the batch
    that reaches it by the default plan is in the hundreds, so GPMPC_PAIR_SB=1 GPMPC_TILING=4 ask for it at B = 5 (odd: a half-empty last wave).
    Balanced runs (pack.hip: work list 7, D >= 6, built when the 64-column tiles of ONE trajectory exceed 1.1 workgroup generations of 4 per CU
    less 2 ds): at ds = 6 that is 6 x sum over tile rows of ceil(span / 64) > 1113, first true at Np = 2368 (1140 tiles): N = 2310, the default
    plan of B = 1.  (tests/test_gpu_fullsize.py runs the list at N = 2500 ... 4096.)"""
    cfg, N, ds, da, H, B = OG.WIDE_CASES[tag]
    args = (cfg, N, ds, da, H, B, False)
    pb, kinv = OG.problem(*args)
    pack, cost = _pack(G, pb, kinv), _cost(G, pb)
    env, assert_plan = OG.wide_step(tag)
    with _tuning(pack, env):
        plan = pack.plan(B, H)
        assert_plan(plan)
        _run_diag(G, pack, pb, cost, B, args, -1.0, "%s N=%d ds=%d B=%d %s" % (tag, N, ds, B, plan["form"]))
    del pack
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. one lambda for all GPs, one amplitude per GP
# ------------------------------------------------------------------------------------------------------------------------------
def _close_forms(a, b, what):
    """Two forms of the same sums (tests/test_gpu_shared_lambda.py: the exponent rounded the same way, partial sums cut differently)."""
    np.testing.assert_allclose(a["means"], b["means"], rtol=1e-9, atol=1e-12, err_msg=what)
    np.testing.assert_allclose(a["vars"], b["vars"], rtol=1e-6, atol=1e-14, err_msg=what)
    np.testing.assert_allclose(a["grad"], b["grad"], rtol=1e-5, atol=1e-9, err_msg=what)


@pytest.mark.parametrize("ds,da", OG.SHARED_DIMS)
def test_shared_lambda_forms_with_distinct_sigma_f(G, ds, da):
    """The pack detects bit-identical length-scales whatever the amplitudes; its forms evaluate exponent and exp once per pair for a GROUP of GPs
    (2; 3; 4, or 2 + 2 on the split list; 3 + 2) and must still weigh each GP with its own sf: fused_sb_shared, head+pair_sbs on the 256x64 and
    the 256x256 shared lists, the whole-horizon kernel over units of two GPs and over all GPs in one unit (ds = 3, 4).  Each against the C port
    (which knows nothing of shared length-scales) and against the same pack with GPMPC_SHARED=0."""
    D = ds + da
    bs = OG.shared_batches(ds)
    args = (OG.shared_config(ds, da), OG.LADDER_N, ds, da, OG.LADDER_H, max(bs.values()), True)
    pb, kinv = OG.problem(*args)
    H = pb["H"]
    assert len(set(pb["sigma_f"])) == ds and np.all(pb["lambdas"] == pb["lambdas"][0])
    pack, cost = _pack(G, pb, kinv), _cost(G, pb)
    assert pack.shared_lambda                                 # detection looks at the length-scales alone
    lam = pb["lambdas"].copy()
    lam[ds - 1, 0] = np.nextafter(lam[ds - 1, 0], 10.0)
    assert not G.GPPack(pb["X"], pb["Y"], kinv, lam, pb["sigma_f"]).shared_lambda
    steps = OG.shared_steps(ds)                              # (B, overrides, form, tiling, how the kernel name shows it)
    reached = set()
    for B, env, form, tiling, kern in steps:
        what = "shared ds=%d da=%d B=%d %s %s %s" % (ds, da, B, form, tiling, kern)
        with _tuning(pack, env):
            plan = pack.plan(B, H)
            OG.assert_shared_plan(plan, (B, env, form, tiling, kern))
            r = _run_diag(G, pack, pb, cost, B, args, -1.0, what)
        with _tuning(pack, dict(env, GPMPC_SHARED="0")):
            plan0 = pack.plan(B, H)
            assert plan0["shared"] == 0 and "shared" not in plan0["form"] and plan0["form"] != "head+pair_sbs", plan0
            if form == "persist":
                assert plan0["form"] == "persist" and ",1>x" in plan0["kernel"], plan0
            d = _np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost))
        _close_forms(r, d, what + " vs GPMPC_SHARED=0 (" + plan0["form"] + ")")
        reached.add((form, tiling, kern))
    print(sorted(reached))
    assert reached == {(s[2], s[3], s[4]) for s in steps}


# ------------------------------------------------------------------------------------------------------------------------------
# 3. full covariance
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", OG.FULLCOV_CASES, ids=lambda c: "ds%d-da%d-N%d%s" % (c[2], c[3], c[1], "-shared" if c[4] else ""))
def test_fullcov_rollout_vs_cport(G, case):
    """test_fullcov_rollout_every_shape_vs_cport and test_fullcov_rollout_with_one_lambda_vs_cport (tests/test_gpu_instances.py) off the grid:
    the two-launch form on each of its tilings and the four-launch form at a small and a large batch (staged kernel | pair_kernel_sbf.h); with one
    lambda, the cross-unit kernel pair_kernel_sbfx.h (ds <= 4; its weights are beta_a,i beta_b,j, which carry sf_a^2 sf_b^2) and its per-unit
    fallback (ds = 5), and the same pack with the sharing off.  Means, full covariances, cost, directional derivatives."""
    cfg, N, ds, da, shared = case
    H, b_big = OG.FULLCOV_H, OG.fullcov_big_batch(ds)
    args = (cfg, N, ds, da, H, b_big, shared)
    pb, kinv = OG.problem(*args)
    pack, cost = _pack(G, pb, kinv), _cost(G, pb)
    pack.enable_fullcov()
    cases = OG.fullcov_steps(ds, shared)                     # (B, overrides, form)
    if shared:                                               # (a pack with da >= 3 has no kernel that shares the exponent and does not report one lambda)
        assert np.all(pb["lambdas"] == pb["lambdas"][0]) and pack.shared_lambda == (da <= 2)
    res = {}
    for B, env, form in cases:
        what = "fullcov ds=%d da=%d N=%d B=%d %s" % (ds, da, N, B, env or "default")
        pick = OG.picks(B)
        ref = _ref_fullcov(args, pick)
        with _tuning(pack, env):
            plan = pack.plan_fullcov(B, H)
            what += OG.assert_fullcov_plan(plan, (B, env, form), ds, da)
            r = G.rollout_fullcov(pack, pb["x0"][:B], pb["U"][:B], cost)
            f = G.rollout_fullcov(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=False)
        _check_fullcov(r, ref, pick, what)
        _check_fullcov(f, ref, pick, what + " objective only", grad=False)
        res[(B, tuple(sorted(env.items())))] = _np(r)
    if shared:                                                # the sharing forced on and switched off: the same sums, cut differently
        with _tuning(pack, {"GPMPC_FC_SHARED": "0"}):
            assert pack.plan_fullcov(3, H)["shared_cross_units"] == 0
            u = _np(G.rollout_fullcov(pack, pb["x0"][:3], pb["U"][:3], cost))
        r = res[(3, (("GPMPC_FC_SHARED", "1"),))]
        for key in ("means", "covs", "cost", "grad"):             # (tests/test_gpu_instances.py: half the tolerance against the C port)
            np.testing.assert_allclose(r[key], u[key], rtol=5e-5, atol=1e-7 * np.abs(u[key]).max(), err_msg=key)


def test_moment_match_full_S_at_D6_through_the_large_batch_kernel(G):
    """gpmpc_moment_match with a FULL input covariance at D = 6 (ds = 3, da = 3): a small batch (staged kernel) and one large enough for
    pair_kernel_sbf.h -- moment.hip::plan_mom takes it from ceil(nq / 2) x units >= 1536 workgroups for a padded size that is no multiple of 256
    (N = 90 pads to 128; 6 units with the cross-covariances: nq = 515) -- against the C port's single step at distinct amplitudes."""
    from oracle import cport
    D, ds = 6, 3
    args = (96, 90, ds, D - ds, 1, 1, False)
    pb, kinv = OG.problem(*args)
    pack = _pack(G, pb, kinv).enable_fullcov()
    units = ds + ds * (ds - 1) // 2
    rng = np.random.default_rng(D)
    for nq in (2, 2 * (-(-1536 // units)) + 3):
        u = 0.5 * rng.normal(size=(nq, D))
        A = rng.normal(size=(nq, D, D))
        S = 0.02 * A @ np.swapaxes(A, 1, 2) + 0.01 * np.eye(D)
        r = _np(G.moment_match(pack, u, S, want_cov=True, want_grad=True))
        assert all(np.all(np.isfinite(v)) for v in r.values())
        for q in OG.picks(nq):
            m, c = cport.moment_match_fullcov(pb["X"], kinv, pb["Y"], pb["lambdas"], pb["sigma_f"], u[q], S[q], nthreads=4)
            assert np.linalg.eigvalsh(c).min() > 0
            m1, c1 = cport.moment_match_fullcov(pb["X"], OG.with_sigma_f(pb, np.ones(ds))[1], pb["Y"], pb["lambdas"], np.ones(ds), u[q], S[q], nthreads=4)
            assert _excess(m1, m, MEAN_RTOL, 1e-9) > 100 or _excess(c1, c, VAR_RTOL, 1e-6 * np.abs(c).max()) > 100      # the amplitudes matter here
            print("DEV moment_match full S D=6 nq=%d [%d]: mean %.3g cov %.3g of the tolerance" % (
                nq, q, _excess(r["mean"][q], m, MEAN_RTOL, 1e-9), _excess(r["cov"][q], c, VAR_RTOL, 1e-6 * np.abs(c).max())))
            np.testing.assert_allclose(r["mean"][q], m, rtol=MEAN_RTOL, atol=1e-9)
            np.testing.assert_allclose(r["cov"][q], c, rtol=VAR_RTOL, atol=1e-6 * np.abs(c).max())
            np.testing.assert_allclose(r["var"][q], np.diag(c), rtol=VAR_RTOL)


def test_moment_match_diagonal_S_on_a_large_batch(G):
    """The single-step entry on DIAGONAL input covariances at a batch that plan_mom sends through the large-tile pair kernel (N = 150 pads to 192:
    ceil(nq / 2) x ds >= 1536 workgroups -> nq = 1027 at ds = 3), and at nq = 2 (staged kernel): the existing single-step cases with sigma_f away
    from 1 (g1 "c", g2) run small batches only."""
    from oracle import cport
    ds, da = 3, 1
    D = ds + da
    args = (97, 150, ds, da, 1, 1, False)
    pb, kinv = OG.problem(*args)
    pack = _pack(G, pb, kinv)
    kinv1 = OG.with_sigma_f(pb, np.ones(ds))[1]
    rng = np.random.default_rng(97)
    for nq in (2, 2 * (-(-1536 // ds)) + 3):
        u = 0.7 * rng.normal(size=(nq, D))
        S = np.zeros((nq, D, D))
        S[:, np.arange(D), np.arange(D)] = rng.uniform(1e-3, 0.05, size=(nq, D))
        r = _np(G.moment_match(pack, u, S))
        assert all(np.all(np.isfinite(v)) for v in r.values())
        for q in OG.picks(nq):
            m, c = cport.moment_match_fullcov(pb["X"], kinv, pb["Y"], pb["lambdas"], pb["sigma_f"], u[q], S[q], nthreads=4)
            assert np.all(np.diag(c) > 0)
            m1, c1 = cport.moment_match_fullcov(pb["X"], kinv1, pb["Y"], pb["lambdas"], np.ones(ds), u[q], S[q], nthreads=4)
            assert _excess(m1, m, MEAN_RTOL, 1e-9) > 100 or _excess(np.diag(c1), np.diag(c), VAR_RTOL, 0.0) > 100
            print("DEV moment_match diagonal S nq=%d [%d]: mean %.3g var %.3g of the tolerance" % (
                nq, q, _excess(r["mean"][q], m, MEAN_RTOL, 1e-9), _excess(r["var"][q], np.diag(c), VAR_RTOL, 0.0)))
            np.testing.assert_allclose(r["mean"][q], m, rtol=MEAN_RTOL, atol=1e-9)
            np.testing.assert_allclose(r["var"][q], np.diag(c), rtol=VAR_RTOL)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. packs with a linear nominal model
# ------------------------------------------------------------------------------------------------------------------------------
NOMINAL_CASES = {"c1": OG.DIAG_CASES[0], "c3": OG.DIAG_CASES[2], "c3s": OG.DIAG_CASES[3]}
NOMINAL_FORMS = {"c1": {"head+pair_staged"}, "c3": {"head+pair_staged", "head+pair_sb"}, "c3s": {"head+pair_staged", "head+pair_sbs"}}
BMAX = 64


def _nominal_ref(tag, b):
    """Trajectory b by tests/nominal_reference.py (oracle + autograd), once per module.  (0.3 ... 2 s each: the first and the last trajectory of a
    batch are compared, as tests/test_gpu_nominal.py does.)"""
    if ("n", tag, b) not in _refs:
        from oracle import gpmpc_oracle as O
        cfg, N, ds, da, H, shared, gamma = NOMINAL_CASES[tag]
        pb, kinv = OG.problem(cfg, N, ds, da, H, BMAX, shared)
        gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"], Ky_inv=kinv)
        W, c = synth_nominal(ds, da)
        r = nominal_rollout(gp, W, c, H, pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], gamma)
        assert_reference_is_sane(r, pb["Q"], gamma)
        _refs[("n", tag, b)] = r
    return _refs[("n", tag, b)]


@pytest.mark.parametrize("tag", ["c1", "c3", "c3s"])
def test_nominal_packs_vs_reference(G, tag):
    """Cases "c1", "c3", "c3s" of tests/test_gpu_nominal.py off the grid, B = 1 and 64: the nominal twins of the head / tail kernels
    (var = sf^2 - T - mu^2 plus the linear terms) under all three two-launch forms, and the solver callback."""
    cfg, N, ds, da, H, shared, gamma = NOMINAL_CASES[tag]
    pb, kinv = OG.problem(cfg, N, ds, da, H, BMAX, shared)
    pack, cost = _pack(G, pb, kinv, nominal=synth_nominal(ds, da)), _cost(G, pb, gamma)
    forms = set()
    for B, env in ((1, {}), (BMAX, {}), (BMAX, {"GPMPC_PAIR_SB": "0"})):
        with _tuning(pack, env):
            plan = pack.plan(B, H)
            assert plan.get("nominal") == 1 and plan["launches_per_step"] == 2 and plan["form"].startswith("head+pair"), plan
            if env:
                assert plan["form"] == "head+pair_staged", plan
            forms.add(plan["form"])
            r = _np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost))
            f = _np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=False))
        pick = sorted({0, B - 1})
        refs = [_nominal_ref(tag, b) for b in pick]
        ref = {k: np.stack([np.asarray(x[k]) for x in refs]) for k in ("means", "vars", "cost", "grad")}
        _check_diag(r, ref, pick, "nominal %s B=%d %s" % (tag, B, plan["form"]))
        _check_diag(f, ref, pick, "nominal %s B=%d %s objective only" % (tag, B, plan["form"]), grad=False)
    print(sorted(forms))
    assert forms == NOMINAL_FORMS[tag], forms
    for b in (0, BMAX - 1):                                   # the solver callback: host in, host out, captured graph
        ref = _nominal_ref(tag, b)
        cg = pack.objective_gradient(pb["x0"][b], pb["U"][b], cost)
        print("DEV nominal %s callback [%d]: cost %.3g of the tolerance" % (tag, b, abs(cg[0] - ref["cost"]) / abs(ref["cost"]) / COST_RTOL))
        np.testing.assert_allclose(cg[0], ref["cost"], rtol=COST_RTOL)
        _assert_grad(cg[1:], ref["grad"], "nominal %s callback [%d]" % (tag, b))
        np.testing.assert_allclose(pack.objective_gradient(pb["x0"][b], pb["U"][b], cost, want_grad=False)[0], ref["cost"], rtol=COST_RTOL)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. step Jacobians and chance constraints
# ------------------------------------------------------------------------------------------------------------------------------
K95 = 1.6448536269514722


def _rows(ds):
    """The three rows of tests/test_gpu_constraints.py: an axis row at 95 %, a general row at kappa = 2, a general mean-only row."""
    rng = np.random.default_rng(77 + ds)
    A = rng.standard_normal((3, ds))
    A[0] = 0.0
    A[0, 0] = 1.0
    return A, np.array([0.5, 0.2, 0.1]), np.array([K95, 2.0, 0.0])


def _jac_ref(tag, b):
    if ("j", tag, b) not in _refs:
        from oracle import gpmpc_oracle as O
        cfg, N, ds, da, H, shared, gamma = OG.JAC_CASES[tag]
        pb, kinv = OG.problem(cfg, N, ds, da, H, 2, shared)
        gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"], Ky_inv=kinv)
        r = reference_constraints(gp, H, pb["x0"][b], pb["U"][b], *_rows(ds))
        OG.assert_diag_reference_is_sane(r["means"], r["vars"], 0.0, pb["Q"], gamma)
        assert np.all(np.isfinite(r["jac"]))
        _refs[("j", tag, b)] = r
    return _refs[("j", tag, b)]


@pytest.mark.parametrize("mode", ["default", "two_launch"])
@pytest.mark.parametrize("tag", ["c3", "d6"])
def test_rollout_jacobians_and_constraints_vs_reference(G, tag, mode):
    """gpmpc_rollout_jac (the step Jacobians d(mu, var)_t / d(mu, var, u)_t-1, each with its own sf factors) through the chance constraints and
    their dense Jacobian, which chain ALL of them: gpmpc_rollout_constraints on gpmpc_rollout_jac's output, and gpmpc_rollout_constrained in
    one pass, against tests/constraints_reference.py (autograd row by row); tolerances of tests/test_gpu_constraints.py."""
    from gaussian_process_mpc_amd._lib import lib, check, ptr, stream_ptr
    cfg, N, ds, da, H, shared, gamma = OG.JAC_CASES[tag]
    B = 2
    pb, kinv = OG.problem(cfg, N, ds, da, H, B, shared)
    A, bb, kap = _rows(ds)
    sc, cost = G.StateConstraints(A, bb, kappa=kap), _cost(G, pb, gamma)
    force = {k: "0" for k in ("GPMPC_FUSED", "GPMPC_FUSED_SB", "GPMPC_PERSIST")} if mode == "two_launch" else {}
    pack = _pack(G, pb, kinv)
    with _tuning(pack, force):
        plan = pack.plan(B, H)
        if mode == "default":
            assert plan["launches_per_step"] in (0, 1) and (plan["form"].startswith("fused") or plan["form"] == "persist"), plan
        else:
            assert plan["launches_per_step"] == 2 and plan["form"].startswith("head+pair"), plan
        dev = pack.device
        x0, U = torch.as_tensor(pb["x0"][:B], device=dev), torch.as_tensor(pb["U"][:B], device=dev)
        e = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)  # noqa: E731
        means, vars_, jac = e(B, H + 1, ds), e(B, H + 1, ds), e(B, H, 2 * ds, 2 * ds + da)
        ws = pack.workspace(lib().gpmpc_rollout_jac_workspace_bytes(pack.handle, B, H))
        check(lib().gpmpc_rollout_jac(pack.handle, B, H, ptr(x0), ptr(U), ptr(means), ptr(vars_), ptr(jac), ctypes.c_void_p(ws.data_ptr()),
                                      ws.numel(), stream_ptr()), "gpmpc_rollout_jac")
        torch.cuda.synchronize()
        assert torch.isfinite(jac).all()
        pure = _np(G.rollout_constraints(means, vars_, jac, sc, ds, da))
        one = _np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=True, constraints=sc))
    means, vars_ = means.cpu().numpy(), vars_.cpu().numpy()
    for b in (B - 1,):                                        # (a reference Jacobian takes 3 ... 4 s of autograd: one trajectory per case, not the first)
        ref = _jac_ref(tag, b)
        what = "jacobians %s %s [%d] %s" % (tag, mode, b, plan["form"])
        tol = 1e-5 * (np.abs(ref["means"][1:, None, :] * A[None, :, :])).sum(axis=2) + 0.5e-4 * kap[None, :] * ref["sd"] + 1e-9
        for name, got in (("gpmpc_rollout_jac + gpmpc_rollout_constraints", pure), ("gpmpc_rollout_constrained", one)):
            err = np.abs(got["g"][b] - ref["g"])
            jerr = np.linalg.norm(got["g_jac"][b] - ref["jac"]) / np.linalg.norm(ref["jac"])
            print("DEV %s %s: g %.3g, dense Jacobian %.3g of the tolerance" % (what, name, (err / tol).max(), jerr / GRAD_RTOL))
            assert np.all(err <= tol), (what, name, err.max())
            for i in range(H * 3):
                _assert_grad(got["g_jac"][b][i], ref["jac"][i], "%s %s row %d" % (what, name, i))
            _assert_grad(got["g_jac"][b], ref["jac"], "%s %s whole matrix" % (what, name))
        np.testing.assert_allclose(means[b], ref["means"], rtol=MEAN_RTOL, atol=1e-9, err_msg=what)
        np.testing.assert_allclose(vars_[b], ref["vars"], rtol=VAR_RTOL, atol=1e-12, err_msg=what)
        np.testing.assert_allclose(one["means"][b], ref["means"], rtol=MEAN_RTOL, atol=1e-9, err_msg=what)
        np.testing.assert_allclose(one["vars"][b], ref["vars"], rtol=VAR_RTOL, atol=1e-12, err_msg=what)


# ------------------------------------------------------------------------------------------------------------------------------
# 6. life cycle: the amplitudes follow GPPack.rebuild
# ------------------------------------------------------------------------------------------------------------------------------
def test_rebuild_replaces_the_amplitudes_everywhere(G):
    """A pack built at sigma_f = 1 and run (eagerly, and on a graph that stays captured), refilled in place with the off-grid amplitudes (same X / Y,
    new Ky_inv): equal to a fresh pack bit for bit, eagerly and on the graph captured BEFORE the refill -- no folded weight, mean factor or
    constant of the old amplitudes survives --; and back to 1: the first results again, bit for bit."""
    cfg, N, ds, da, H, shared, gamma = OG.DIAG_CASES[0]
    B = 3
    args = (cfg, N, ds, da, H, BMAX, shared)
    pb, kinv = OG.problem(*args)
    one, kinv1 = OG.with_sigma_f(pb, np.ones(ds))
    cost = _cost(G, pb, gamma)
    x0, U = pb["x0"][:B], pb["U"][:B]
    pack = G.GPPack(pb["X"], pb["Y"], kinv1, pb["lambdas"], one["sigma_f"])
    e1, g1 = _np(G.rollout(pack, x0, U, cost)), _np(G.rollout(pack, x0, U, cost, graph=True))
    g1 = _np(G.rollout(pack, x0, U, cost, graph=True))                       # (the replay)
    cb1 = pack.objective_gradient(x0[0], U[0], cost).copy()
    h = pack.handle
    assert pack.rebuild(pb["X"], pb["Y"], kinv, pb["lambdas"], pb["sigma_f"]) and pack.handle is h
    fresh = _np(G.rollout(_pack(G, pb, kinv), x0, U, cost))
    e2, g2 = _np(G.rollout(pack, x0, U, cost)), _np(G.rollout(pack, x0, U, cost, graph=True))
    cb2 = pack.objective_gradient(x0[0], U[0], cost).copy()
    for k in ("means", "vars", "cost", "grad"):
        assert np.array_equal(e2[k], fresh[k]) and np.array_equal(g2[k], fresh[k]), k
        assert not np.array_equal(e2[k][..., 1:, :] if k in ("means", "vars") else e2[k], e1[k][..., 1:, :] if k in ("means", "vars") else e1[k]), k
    _check_diag(e2, _ref_diag(args, gamma, OG.picks(B)), OG.picks(B), "after rebuild with the off-grid amplitudes")
    np.testing.assert_allclose(cb2[0], fresh["cost"][0], rtol=1e-10)
    assert pack.rebuild(pb["X"], pb["Y"], kinv1, pb["lambdas"], one["sigma_f"]) and pack.handle is h
    e3, g3 = _np(G.rollout(pack, x0, U, cost)), _np(G.rollout(pack, x0, U, cost, graph=True))
    cb3 = pack.objective_gradient(x0[0], U[0], cost).copy()
    for k in ("means", "vars", "cost", "grad"):
        assert np.array_equal(e3[k], e1[k]) and np.array_equal(g3[k], g1[k]) and np.array_equal(g1[k], e1[k]), k
    assert np.array_equal(cb3, cb1) and not np.array_equal(cb2, cb1)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. the class path: Dynamics + RiskSensitiveMPC over GPs with their own amplitudes
# ------------------------------------------------------------------------------------------------------------------------------
def test_mpc_callbacks_with_distinct_sigma_f_references_and_input_rate_cost(G):
    """Dynamics gathers lambdas / sigma_f of its GPs into the pack (dynamics.py), RiskSensitiveMPC hands x_ref, u_ref, R_delta and last_u to the
    cost: N = 100, ds = 2, da = 2, H = 10, set_sigma_f with a different value per GP.  objective / gradient callbacks and the batched evaluation
    against oracle.objective_and_gradient(..., R_delta=, last_u=) on the Ky_inv the GPs built themselves."""
    from oracle import gpmpc_oracle as O
    cfg, N, ds, da, H, shared, gamma = OG.DIAG_CASES[0]
    pb, _ = OG.problem(cfg, N, ds, da, H, BMAX, shared)
    rng = np.random.default_rng(5)
    Rd = 0.05 * np.eye(da) + 0.01 * (np.ones((da, da)) - np.eye(da))
    mpc = G.RiskSensitiveMPC(gamma, H, ds, da, pb["Q"], pb["R"], Rd)
    for a, g in enumerate(mpc.dynamics.gpr_err):
        g.set_lambdas(pb["lambdas"][a])
        g.set_sigma_n(np.array(pb["sigma_n"][a]))
        g.set_sigma_f(np.array(pb["sigma_f"][a]))             # (float64 arrays: exact logs)
    mpc.dynamics.append_train_data(pb["X"][:, :ds], pb["X"][:, ds:], pb["Y"])
    mpc.set_xref(pb["x_ref"])
    mpc.set_uref(pb["u_ref"])
    mpc.last_traj = rng.uniform(-1, 1, H * da)
    last_u = mpc.last_traj[:da].copy()
    np.testing.assert_allclose([g.get_sigma_f() for g in mpc.dynamics.gpr_err], pb["sigma_f"], rtol=1e-15)
    np.testing.assert_allclose(mpc.dynamics.pack().sigma_f, pb["sigma_f"], rtol=1e-15)
    Kinv = torch.stack([g.Ky_inv.detach().cpu() for g in mpc.dynamics.gpr_err])
    gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"], Ky_inv=Kinv)
    B = 3
    refs = []
    for b in range(B):
        o = O.objective_and_gradient(gp, H, pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], gamma, R_delta=Rd, last_u=last_u, mode="o2")
        OG.assert_diag_reference_is_sane(o["means"], o["vars"], o["cost"], pb["Q"], gamma)
        plain = O.objective_and_gradient(gp, H, pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], gamma, mode="o2", want_grad=False)
        assert abs(plain["cost"] - o["cost"]) > 100 * COST_RTOL * abs(o["cost"])       # the input-rate term matters
        refs.append(o)
    for b in range(B):
        mpc.curr_state = torch.tensor(pb["x0"][b], dtype=torch.float64, device=mpc.device)
        mpc._cache_key = None
        x = pb["U"][b].reshape(-1).copy()
        c, g = mpc.objective(x), mpc.gradient(x)
        print("DEV class path callbacks [%d]: cost %.3g of the tolerance" % (b, abs(c - refs[b]["cost"]) / abs(refs[b]["cost"]) / COST_RTOL))
        np.testing.assert_allclose(c, refs[b]["cost"], rtol=COST_RTOL)
        _assert_grad(g, refs[b]["grad"], "class path callbacks [%d]" % b)
    r = _np(mpc.evaluate_batch(torch.as_tensor(pb["U"][:B], device=mpc.device), curr_state=torch.as_tensor(pb["x0"][:B], device=mpc.device)))
    ref = {k: np.stack([np.asarray(o[k]) for o in refs]) for k in ("means", "vars", "cost", "grad")}
    _check_diag(r, ref, list(range(B)), "class path evaluate_batch")


# ------------------------------------------------------------------------------------------------------------------------------
# 8. action_dim >= 3: the default plan of every plant with three or more inputs (csrc/plan.hip: head kernel + staged pair_kernel.h + tail
#    kernel at every batch; fullcov.hip: the four-launch form at every batch)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds,da,N", OG.WIDEACT_CASES, ids=["ds%d-da%d-N%d" % c for c in OG.WIDEACT_CASES])
def test_wide_action_ladder_vs_cport(G, ds, da, N):
    """Every D from 4 to 8 at da >= 3 (N = 150: Np = 192), each plan asserted from ``pack.plan``: the staged fp64 kernel on 64x64 tiles with one,
    two (odd batch, eager and as a captured graph) and four (4 + 1) trajectories per workgroup, on the 256x256 list from ceil(B / 2) ds >= 1024 with
    two (odd batch) and one; the tail sweep over da >= 3 columns per step Jacobian.  The long case (N = 1415: Np = 1472) runs the 64x128 list
    behind a head kernel in row chunks.  Objective + gradient and objective only, against cport.rollout."""
    D = ds + da
    args, steps, expected = OG.wideact_case(ds, da, N)
    pb, kinv = OG.problem(*args)
    H = pb["H"]
    pack, cost = _pack(G, pb, kinv), _cost(G, pb)
    reached = set()
    for step in steps:
        B, env, form, tiling, tb, mode = step
        graph = mode == "graph"
        with _tuning(pack, env):
            plan = pack.plan(B, H, graph=graph)
            OG.assert_wideact_plan(plan, step, D)
            OG.assert_wideact_plan(pack.plan(B, H, want_grad=False, graph=graph), step, D)
            _run_diag(G, pack, pb, cost, B, args, -1.0, "wideact ds=%d da=%d N=%d B=%d %s %s tb=%d %s" % (ds, da, N, B, form, tiling, tb, mode), graph=graph)
        reached.add(step[2:])
    print(sorted(reached))
    assert reached == expected, reached ^ expected
    del pack
    torch.cuda.empty_cache()


@pytest.mark.parametrize("ds,da", OG.WIDEACT_INERT_DIMS)
def test_wide_action_overrides_are_inert(G, ds, da):
    """Overrides that select among kernels a da >= 3 pack does not have (whole-horizon, fused, scalar-broadcast, their tilings, the step-1 quadratic
    form) leave the plan what it was -- head+pair_staged on the same tiling, no step1=quad -- and, the same kernel on the same work list, every
    bit of the result."""
    D = ds + da
    bs = OG.wideact_batches(ds)
    args, steps, _ = OG.wideact_case(ds, da, OG.LADDER_N)
    pb, kinv = OG.problem(*args)
    H = pb["H"]
    pack, cost = _pack(G, pb, kinv), _cost(G, pb)
    for step in steps:
        B, env, form, tiling, tb, mode = step
        if env or mode == "graph" or B not in (bs["small"], bs["big"]):
            continue
        OG.assert_wideact_plan(pack.plan(B, H), step, D)
        base = _np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost))
        _check_diag(base, _ref_diag(args, -1.0, OG.picks(B)), OG.picks(B), "wideact inert ds=%d da=%d B=%d default" % (ds, da, B))
        for over in OG.WIDEACT_INERT:
            with _tuning(pack, over):
                OG.assert_wideact_plan(pack.plan(B, H), step, D)
                r = _np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost))
            for k in ("means", "vars", "cost", "grad"):
                assert np.array_equal(r[k], base[k]), (over, B, k)


@pytest.mark.parametrize("case", OG.WIDEACT_FULLCOV, ids=lambda c: "ds%d-da%d-N%d%s" % (c[2], c[3], c[1], "-shared" if c[4] else ""))
def test_wide_action_fullcov_vs_cport(G, case):
    """test_fullcov_rollout_vs_cport at da >= 3, step for step: the two-launch form has no instance there, so every step -- GPMPC_FC_FORM, _TILING
    and _SHARED included -- must plan and run the four-launch form (staged kernel at the small batches, pair_kernel_sbf.h at the large one) with
    per-unit cross terms, also on the pack with one lambda.  Means, covariances, cost, complex-step directional derivatives of the C port."""
    test_fullcov_rollout_vs_cport(G, case)


def _model_ref(kind, args, b):
    """Trajectory b of a WIDEACT_MODEL problem by the reference of its kind, once per module, sanity re-asserted."""
    if (kind, args, b) not in _refs:
        import noise_reference as NR
        from oracle import gpmpc_oracle as O
        pb, kinv = OG.problem(*args)
        ds, da, H = pb["ds"], pb["da"], pb["H"]
        gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"], Ky_inv=kinv)
        common = (H, pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], -1.0)
        if kind == "nominal":
            r = nominal_rollout(gp, *synth_nominal(ds, da), *common)
        elif kind == "noise":
            P, av, w = NR.ladder_noise(ds, da)
            r = NR.rollout(gp, *common, init_cov=P, action_var=av, process_var=w)
        else:
            r = reference_constraints(gp, H, pb["x0"][b], pb["U"][b], *_rows(ds))
            assert np.all(np.isfinite(r["jac"]))
        OG.assert_diag_reference_is_sane(r["means"], r["vars"], r.get("cost", 0.0), pb["Q"], -1.0)
        _refs[(kind, args, b)] = r
    return _refs[(kind, args, b)]


@pytest.mark.parametrize("kind", ["nominal", "noise"])
@pytest.mark.parametrize("case", OG.WIDEACT_MODEL, ids=lambda c: "ds%d-da%d" % (c[2], c[3]))
def test_wide_action_nominal_and_noise_models_vs_reference(G, case, kind):
    """da >= 3 through the head / tail kernels' other variants: a pack with a linear nominal model (k_roll_head<D, 1 | 2>: with and without
    gradient) against tests/nominal_reference.py; a pack under a noise model -- init_cov with off-diagonal entries, a different action_var per
    action (the first exactly 0), process_var > 0: the offsets of the noise image behind da >= 3 action variances -- against
    tests/noise_reference.py.  B = 1, 2, 5; objective + gradient and objective only."""
    import noise_reference as NR
    cfg, N, ds, da, H = case
    args = (cfg, N, ds, da, H, max(OG.WIDEACT_MODEL_B), False)
    pb, kinv = OG.problem(*args)
    cost = _cost(G, pb)
    if kind == "nominal":
        pack = _pack(G, pb, kinv, nominal=synth_nominal(ds, da))
    else:
        P, av, w = NR.ladder_noise(ds, da)
        assert np.abs(P - np.diag(np.diag(P))).max() > 0 and len(set(av)) == da and np.all(w > 0)
        pack = _pack(G, pb, kinv).set_noise(init_cov=P, action_var=av, process_var=w)
        assert not pack.noise_is_default
    for B in OG.WIDEACT_MODEL_B:
        plan = pack.plan(B, H)
        assert plan["form"] == "head+pair_staged" and "gpmpc_pair_kernel<%d,true," % (ds + da) in plan["kernel"] and plan["tb"] == min(B, 2), plan
        assert (plan.get("nominal") == 1) == (kind == "nominal"), plan
        r = _np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost))
        f = _np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=False))
        pick = OG.picks(B)
        refs = [_model_ref(kind, args, b) for b in pick]
        ref = {k: np.stack([np.asarray(x[k]) for x in refs]) for k in ("means", "vars", "cost", "grad")}
        _check_diag(r, ref, pick, "wideact %s ds=%d da=%d B=%d" % (kind, ds, da, B))
        _check_diag(f, ref, pick, "wideact %s ds=%d da=%d B=%d objective only" % (kind, ds, da, B), grad=False)


@pytest.mark.parametrize("case", OG.WIDEACT_MODEL, ids=lambda c: "ds%d-da%d" % (c[2], c[3]))
def test_wide_action_jacobians_and_constraints_vs_reference(G, case):
    """gpmpc_rollout_jac (step Jacobians with da >= 3 action columns) through gpmpc_rollout_constraints, and gpmpc_rollout_constrained in one pass,
    on the three mixed rows, B = 1, 2, 5, against tests/constraints_reference.py by the criteria of tests/test_gpu_constraints.py -- the
    exact-zero causality blocks, da columns wide, included."""
    import test_gpu_constraints as TC
    cfg, N, ds, da, H = case
    args = (cfg, N, ds, da, H, max(OG.WIDEACT_MODEL_B), False)
    pb, kinv = OG.problem(*args)
    A, bb, kap = _rows(ds)
    sc, cost, pack = G.StateConstraints(A, bb, kappa=kap), _cost(G, pb), _pack(G, pb, kinv)
    for B in OG.WIDEACT_MODEL_B:
        assert pack.plan(B, H)["form"] == "head+pair_staged"
        means, vars_, jac = TC._rollout_jac(pack, pb["x0"][:B], pb["U"][:B])
        assert torch.isfinite(jac).all()
        pure = _np(G.rollout_constraints(means, vars_, jac, sc, ds, da))
        one = _np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=True, constraints=sc))
        val = _np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=False, constraints=sc))
        np.testing.assert_array_equal(val["g"], one["g"])
        means, vars_ = means.cpu().numpy(), vars_.cpu().numpy()
        for b in OG.picks(B):
            ref = _model_ref("constraints", args, b)
            for name, got in (("gpmpc_rollout_jac + gpmpc_rollout_constraints", pure), ("gpmpc_rollout_constrained", one)):
                what = "wideact constraints ds=%d da=%d B=%d [%d] %s" % (ds, da, B, b, name)
                TC._assert_g(got["g"][b], ref, A, kap, what)
                TC._assert_jac(got["g_jac"][b], ref["jac"], H, 3, da, what)
            for m, v in ((means, vars_), (one["means"], one["vars"])):
                np.testing.assert_allclose(m[b], ref["means"], rtol=MEAN_RTOL, atol=1e-9)
                np.testing.assert_allclose(v[b], ref["vars"], rtol=VAR_RTOL, atol=1e-12)


def test_wide_action_autograd_path_equals_the_fused_adjoint(G):
    """autograd.RolloutFunction (gpmpc_rollout_jac + gpmpc_rollout_vjp) at ds = 2, da = 3: u.grad of cost_torch(forward_propagate_torch(...)) against
    the gradient of ``rollout`` on the same pack and cost, 1e-9 relative (tests/test_gpu_autograd.py's tolerance for the same pair)."""
    cfg, N, ds, da, H = OG.WIDEACT_MODEL[0]
    pb, _ = OG.problem(cfg, N, ds, da, H, max(OG.WIDEACT_MODEL_B), False)
    mpc = G.RiskSensitiveMPC(-1.0, H, ds, da, pb["Q"], pb["R"])
    for a, g in enumerate(mpc.dynamics.gpr_err):
        g.set_lambdas(pb["lambdas"][a])
        g.set_sigma_n(np.array(pb["sigma_n"][a]))
        g.set_sigma_f(np.array(pb["sigma_f"][a]))
    mpc.dynamics.append_train_data(pb["X"][:, :ds], pb["X"][:, ds:], pb["Y"])
    mpc.set_xref(pb["x_ref"])
    mpc.set_uref(pb["u_ref"])
    pack, cost = mpc.dynamics.pack(), _cost(G, pb)
    for b in (0, 1):
        x0 = torch.tensor(pb["x0"][b], dtype=torch.float64, device=mpc.device)
        u = torch.as_tensor(pb["U"][b], device=mpc.device).type(torch.float64).requires_grad_(True)
        means, covs = mpc.dynamics.forward_propagate_torch(H, x0, u)
        assert means[1].requires_grad and covs[1].requires_grad
        c = mpc.cost_torch(means, u, covs, mpc.x_ref, mpc.u_ref)
        c.backward()
        r = _np(G.rollout(pack, pb["x0"][b:b + 1], pb["U"][b:b + 1], cost))
        got, ref = u.grad.cpu().numpy(), r["grad"][0]
        print("DEV wideact autograd [%d]: cost %.3g grad %.3g relative" % (b, abs(c.item() - r["cost"][0]) / abs(r["cost"][0]), np.abs(got - ref).max() / np.abs(ref).max()))
        assert got.shape == (H, da) and np.all(np.isfinite(got))
        np.testing.assert_allclose(c.item(), r["cost"][0], rtol=1e-12)
        np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-12)
