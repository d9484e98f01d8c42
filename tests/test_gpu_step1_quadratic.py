"""Horizon step 1 of the two-launch scalar-broadcast form as a quadratic form (csrc/pair_kernel_q1.h, GPMPC_STEP1_QUAD), forced on small
shapes and held against the C port (oracle/cport, ``given_rollout`` / ``given_step_diag`` on the constants the kernels read), against the
FIRST variant of the pair kernel it replaces (the same plan with GPMPC_STEP1_QUAD=0), and to itself (bits).

    shapes   (N, ds, da) = (200, 2, 1)  one row tile, column loop cut by ncol       (449, 4, 1)  partial last tile, diagonal and off-diagonal tiles
                           (200, 3, 2)  two action dimensions                       (130, 6, 1)  D = 7
    batches  B = 17 (three blocks of 8 trajectories, the last one partial), B = 3 and B = 1 (bits of the same trajectories), H = 3 and H = 1
    noise    the defaults | init_cov = 0, action_var = 0 (the step-1 weights equal M) | init_cov = 0.5 I with distinct action_var |
             a full init_cov (the diagonal rollout reads its diagonal)

Tolerances against the C port are the project's (tests/offgrid_problems.py; tests/test_gpu_fullsize.py uses the same numbers).
New against old, step 1: both paths are measured against the long double step on the same constants, K = |error| / (2^-53 A_var) as in
tests/test_gpu_accuracy.py (mu has the same bits on both paths, so the error of the variance IS the error of T = c Z0; A_var is the absolute
sum the cancelling sum is judged by).  Every K stays within the project's budget (OG.BUDGET_K), and IN EACH CASE the new path's K may exceed
the old path's K of the same case by at most Q1_FACTOR = 2.  The factor is determined from these shapes: over the sixteen small cases and the
full-size one the ratio new / old lies between 0.68 and 1.28 (profiles/step1_quad/accuracy.txt) -- both forms round each term to a few ulp, and
which of the two comes out ahead is chance --; 2 is the next round number, about 1.5 x the largest ratio seen.  The kernels sum in a fixed
order, so the figures repeat from run to run.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import offgrid_problems as OG

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
THREADS = 16
Q1_FACTOR = 2.0
FORM = {"GPMPC_PAIR_SB": "1", "GPMPC_FUSED_SB": "0", "GPMPC_PERSIST": "0", "GPMPC_SHARED": "0"}     # head + pair_kernel_sb.h at every batch size
NEW = dict(FORM, GPMPC_STEP1_QUAD="1")
OLD = dict(FORM, GPMPC_STEP1_QUAD="0")
#          config N    ds da
SHAPES = [(31,    200, 2, 1),
          (32,    449, 4, 1),
          (33,    200, 3, 2),
          (34,    130, 6, 1)]
NOISES = ("default", "zero", "large", "full")
B, H = 17, 3
_cases = {}


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    return g


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _noise(name, ds, da):
    """(init_cov, action_var) of a noise model, None = the default of that part."""
    rng = np.random.default_rng(900 + ds)
    if name == "default":
        return None, None
    if name == "zero":
        return np.zeros((ds, ds)), np.zeros(da)
    if name == "large":
        return 0.5 * np.eye(ds), rng.uniform(1e-3, 5e-2, da)
    A = rng.uniform(-1.0, 1.0, (ds, ds))
    return 0.02 * A @ A.T / ds + np.diag(rng.uniform(1e-4, 3e-2, ds)), rng.uniform(1e-4, 1e-2, da)


def _pack(G, pb, kinv, env, noise=(None, None), nominal=None):
    """A pack planned under ``env`` (the overrides are read at creation)."""
    with _env(env):
        pack = G.GPPack(pb["X"], pb["Y"], kinv, pb["lambdas"], pb["sigma_f"], nominal=nominal)
    if noise[0] is not None or noise[1] is not None:
        pack.set_noise(init_cov=noise[0], action_var=noise[1])
    return pack


def _cost(G, pb):
    return G.CostParams(-1.0, pb["Q"], pb["R"], x_ref=pb["x_ref"], u_ref=pb["u_ref"])


def _np(r):
    return {k: v.detach().cpu().numpy().copy() for k, v in r.items()}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b, what):
    for k in b:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k, float(np.max(np.abs(a[k] - b[k]))))


def _roll(G, pack, pb, nb=B, nh=H, **kw):
    return _np(G.rollout(pack, pb["x0"][:nb], pb["U"][:nb, :nh], _cost(G, pb), **kw))


def _takes(pack, nb, nh, quad, grad=True):
    p = pack.plan(nb, nh, want_grad=grad)
    assert p["form"] == "head+pair_sb", p
    assert (p.get("step1") == "quad") == quad, p


def _against_cport(r, c, cg, what):
    np.testing.assert_allclose(r["means"], c["means"], rtol=OG.GPU_MEAN_RTOL, atol=1e-9, err_msg=what)
    np.testing.assert_allclose(r["vars"], c["vars"], rtol=OG.GPU_VAR_RTOL, err_msg=what)
    np.testing.assert_allclose(r["cost"], c["cost"], rtol=OG.GPU_COST_RTOL, err_msg=what)
    if "grad" in r:
        np.testing.assert_allclose(r["grad"], cg["grad"], rtol=OG.GPU_GRAD_RTOL, atol=1e-7, err_msg=what)


def _reference(pb, consts, noise, nb, nh):
    from oracle import cport
    kw = dict(x0=pb["x0"][:nb], U=pb["U"][:nb, :nh], nthreads=THREADS, init_cov=noise[0], action_var=noise[1])
    c = cport.given_rollout(pb, *consts, -1.0, prec="d", **kw)
    OG.assert_diag_reference_is_sane(c["means"], c["vars"][:, 1:], c["cost"], pb["Q"], -1.0)      # (step 0 carries init_cov: zero in one model)
    return c, cport.given_rollout(pb, *consts, -1.0, prec="cd", **kw)


def _k_step1(pb, consts, noise, r, nb=B):
    """K of the variances of step 1 against the long double step on the constants the kernels read."""
    from oracle import cport
    ds, da = pb["ds"], pb["da"]
    s0 = np.full(ds, 1e-3) if noise[0] is None else np.diag(noise[0])
    sa = np.full(da, float(np.float32(1e-3))) if noise[1] is None else noise[1]
    u = np.concatenate([pb["x0"][:nb], pb["U"][:nb, 0]], axis=1)
    s = np.tile(np.concatenate([s0, sa]), (nb, 1))
    ld = cport.given_step_diag(pb, *consts, u, s, prec="ld", nthreads=THREADS)
    assert np.all(np.isfinite(ld["mean"])) and np.all(ld["var"] > 0)
    T = np.abs(pb["sigma_f"] ** 2 - ld["var"] - ld["mean"] ** 2)
    return float(np.max(np.abs(r["vars"][:, 1] - ld["var"]) / (U53 * ld["A_var"]))), float(np.max(ld["A_var"] / T))


def _case(G, shape, noise_name):
    """Both paths at B = 17, H = 3 on one problem and noise model, and K of step 1 for each: computed once, left unchanged."""
    key = (shape, noise_name)
    if key not in _cases:
        cid, N, ds, da = shape
        pb, kinv = OG.problem(cid, N, ds, da, H, B)
        noise = _noise(noise_name, ds, da)
        new, old = _pack(G, pb, kinv, NEW, noise), _pack(G, pb, kinv, OLD, noise)
        _takes(new, B, H, True)
        _takes(old, B, H, False)
        consts = new.beta().cpu().numpy().copy(), new.weights().cpu().numpy()
        rn, ro = _roll(G, new, pb), _roll(G, old, pb)
        kn, amp = _k_step1(pb, consts, noise, rn)
        ko, _ = _k_step1(pb, consts, noise, ro)
        print("Q1ACC N=%d ds=%d da=%d noise=%s: K_var new %.3g old %.3g | A_var/T up to %.3g" % (N, ds, da, noise_name, kn, ko, amp))
        _cases[key] = (pb, noise, new, consts, rn, ro, kn, ko)
    return _cases[key]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_ds%d_da%d" % s[1:])
@pytest.mark.parametrize("noise_name", NOISES)
def test_step1_quadratic_against_cport_and_first_variant(G, shape, noise_name):
    pb, noise, new, consts, rn, ro, kn, ko = _case(G, shape, noise_name)
    c, cg = _reference(pb, consts, noise, B, H)
    _against_cport(rn, c, cg, "new path")
    _against_cport(ro, c, cg, "old path")
    _against_cport(rn, ro, ro, "new against old")
    # the mean sums are the head kernel's on both paths
    assert np.array_equal(_bits(rn["means"][:, 1]), _bits(ro["means"][:, 1]))
    assert kn <= OG.BUDGET_K["var"] and ko <= OG.BUDGET_K["var"], (kn, ko)
    assert kn <= Q1_FACTOR * ko, (kn, ko)
    # partial blocks, other batch sizes: the same trajectories, the same bits
    _same_bits(_roll(G, new, pb), rn, "second call")
    for nb in (3, 1):
        _takes(new, nb, H, True)
        rb = _roll(G, new, pb, nb=nb)
        _same_bits(rb, {k: v[:nb] for k, v in rn.items()}, "B = %d inside B = %d" % (nb, B))
    # H = 1: the step-1 kernel is the only pair launch of the call
    r1 = _roll(G, new, pb, nb=3, nh=1)
    c1, cg1 = _reference(pb, consts, noise, 3, 1)
    _against_cport(r1, c1, cg1, "H = 1")
    assert np.array_equal(_bits(r1["vars"][:, 1]), _bits(rn["vars"][:3, 1]))
    # objective only: the new path takes it too (one moment per tile)
    _takes(new, B, H, True, grad=False)
    rf = _roll(G, new, pb, want_grad=False)
    np.testing.assert_allclose(rf["cost"], c["cost"], rtol=OG.GPU_COST_RTOL)
    assert np.array_equal(_bits(rf["vars"][:, 1]), _bits(rn["vars"][:, 1]))
    # graph replay launches what the plain call launches
    _same_bits(_roll(G, new, pb, graph=True), rn, "graph")


def test_step1_quadratic_accuracy_factor(G):
    """Every case above once more in one place: K of the new path within Q1_FACTOR of K of the old path, case by case."""
    rows = [(shape, noise_name) + _case(G, shape, noise_name)[6:8] for shape in SHAPES for noise_name in NOISES]
    ratios = [r[2] / r[3] for r in rows]
    print("Q1ACC ratio K_var new / old per case: min %.3g max %.3g (allowed %.1f in each case)" % (min(ratios), max(ratios), Q1_FACTOR))
    bad = [r for r in rows if not r[2] <= Q1_FACTOR * r[3]]
    assert not bad, bad


def test_step1_weights_follow_the_pack(G):
    """set_noise, a refill with one more observation (what an append leaves) and with one observation replaced: the next call equals a
    fresh pack, bit for bit -- plainly launched and as the replay of a graph captured before the change."""
    cid, N, ds, da = SHAPES[0]
    pb, kinv = OG.problem(cid, N, ds, da, H, B)
    pb1, kinv1 = OG.problem(cid, N + 1, ds, da, H, B)           # (another draw of N + 1 points: same padded size)
    big = _noise("large", ds, da)
    pack = _pack(G, pb, kinv, NEW)
    for graph in (False, True):
        _roll(G, pack, pb, graph=graph)
    pack.set_noise(init_cov=big[0], action_var=big[1])
    fresh = _roll(G, _pack(G, pb, kinv, NEW, big), pb)
    for graph in (False, True):
        _same_bits(_roll(G, pack, pb, graph=graph), fresh, "after set_noise, graph=%s" % graph)
    # two streams: the call that finds the weights stale refills them on ITS stream; a call on another stream, issued at once, waits for that fill
    pack.set_noise(init_cov=None, action_var=None)
    torch.cuda.synchronize()                                    # (the set is ordered before both streams, as the header asks)
    side = torch.cuda.Stream()
    x0d, Ud = torch.as_tensor(pb["x0"][:B]).cuda(), torch.as_tensor(pb["U"][:B, :H]).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ta = G.rollout(pack, x0d, Ud, _cost(G, pb))
    tb = G.rollout(pack, x0d, Ud, _cost(G, pb))
    torch.cuda.synchronize()
    ra, rb = _np(ta), _np(tb)
    plain = _roll(G, _pack(G, pb, kinv, NEW), pb)
    _same_bits(ra, plain, "the stream that refilled")
    _same_bits(rb, plain, "another stream right behind it")
    pack.set_noise(init_cov=big[0], action_var=big[1])
    assert pack.rebuild(pb1["X"], pb1["Y"], kinv1, pb1["lambdas"], pb1["sigma_f"])
    fresh = _roll(G, _pack(G, pb1, kinv1, NEW, big), pb)
    for graph in (False, True):
        _same_bits(_roll(G, pack, pb, graph=graph), fresh, "after a refill with N + 1 points, graph=%s" % graph)
    X2, Y2 = pb1["X"].copy(), pb1["Y"].copy()
    X2[7], Y2[7] = pb["X"][3], pb["Y"][3]
    from oracle import gpmpc_oracle as O
    kinv2 = O.GPBundle(X2, Y2, pb1["lambdas"], pb1["sigma_f"], pb1["sigma_n"]).Ky_inv.numpy()
    assert pack.rebuild(X2, Y2, kinv2, pb1["lambdas"], pb1["sigma_f"])
    pb2 = dict(pb1, X=X2, Y=Y2)
    fresh = _roll(G, _pack(G, pb2, kinv2, NEW, big), pb)
    for graph in (False, True):
        _same_bits(_roll(G, pack, pb, graph=graph), fresh, "after a replaced point, graph=%s" % graph)


def test_step1_weights_follow_an_append_and_a_replace(G):
    """The online sequence itself: a Dynamics whose pack takes the new path, then one observation appended (C ABI gpmpc_gp_append) and, with the
    window full, one replaced (gpmpc_gp_replace), each followed by the refill of the SAME pack that Dynamics.pack() does.  After each, a rollout
    on that pack equals a fresh pack built from the same GP state, bit for bit, plainly launched and as a graph replay."""
    cid, N, ds, da = SHAPES[0]
    pb, _ = OG.problem(cid, N, ds, da, H, B)
    rng = np.random.default_rng(41)
    dyn = G.Dynamics(ds, da)
    sn = np.broadcast_to(np.asarray(pb["sigma_n"], dtype=np.float64).reshape(-1), (ds,))
    for a, gp in enumerate(dyn.gpr_err):
        gp.set_lambdas(pb["lambdas"][a]); gp.set_sigma_n(np.array(sn[a]))                  # (a lambda per GP: nothing shared)
    dyn.append_train_data(pb["X"][:, :ds], pb["X"][:, ds:], pb["Y"])
    with _env(NEW):
        pack = dyn.pack()                                                                  # (the overrides are read at creation)
    _takes(pack, B, H, True)
    assert not pack.shared_lambda

    def fresh():
        g0 = dyn.gpr_err[0]
        Y = torch.cat([g.y_train.reshape(-1, 1) for g in dyn.gpr_err], dim=1)
        K = torch.stack([g.Ky_inv.detach() for g in dyn.gpr_err]).clone()
        lam, sf = np.stack([g.get_lambdas() for g in dyn.gpr_err]), np.array([g.get_sigma_f() for g in dyn.gpr_err])
        with _env(NEW):
            return _roll(G, G.GPPack(g0.X_train.clone(), Y, K, lam, sf), pb)

    for graph in (False, True):
        _same_bits(_roll(G, pack, pb, graph=graph), fresh(), "before, graph=%s" % graph)
    for what in ("append", "replace"):
        if what == "replace":
            dyn.max_train = N + 1                                                          # the window is full: the next observation replaces slot 0
        s, a = rng.uniform(-1, 1, ds), rng.uniform(-1, 1, da)
        n_before = dyn.gpr_err[0].num_train
        dyn.append_train_data(s, a, s + 0.1 * np.tanh(s), incremental=True)
        assert dyn.gpr_err[0].num_train == (n_before + 1 if what == "append" else n_before)
        assert dyn.pack() is pack                                                          # refilled in place (same padded size)
        ref = fresh()
        for graph in (False, True):
            _same_bits(_roll(G, pack, pb, graph=graph), ref, "after %s, graph=%s" % (what, graph))


def test_nominal_pack_takes_the_new_path(G):
    """A pack with a linear nominal model: the head kernel's nominal variants write the same column values, the step-1 kernel is the same."""
    import nominal_reference as NR
    from oracle import gpmpc_oracle as O
    cid, N, ds, da = SHAPES[1]
    pb, kinv = OG.problem(cid, N, ds, da, H, B)
    W, c = NR.synth_nominal(ds, da)
    gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"], Ky_inv=torch.as_tensor(kinv))
    new, old = _pack(G, pb, kinv, NEW, nominal=(W, c)), _pack(G, pb, kinv, OLD, nominal=(W, c))
    for pack, quad in ((new, True), (old, False)):
        plan = pack.plan(B, H)
        assert plan["form"] == "head+pair_sb" and plan.get("nominal") == 1 and (plan.get("step1") == "quad") == quad, plan
    rn, ro = _roll(G, new, pb), _roll(G, old, pb)
    _against_cport(rn, ro, ro, "nominal, new against old")
    for b in (0, B - 1):
        ref = NR.nominal_rollout(gp, W, c, H, pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], -1.0)
        NR.assert_reference_is_sane(ref, pb["Q"], -1.0)
        _against_cport({k: v[b] for k, v in rn.items()}, ref, ref, "nominal, new path against the reference [%d]" % b)
    _same_bits(_roll(G, new, pb, nb=3), {k: v[:3] for k, v in rn.items()}, "nominal, B = 3 inside B = 17")
    rf = _roll(G, new, pb, want_grad=False)
    assert np.array_equal(_bits(rf["vars"][:, 1]), _bits(rn["vars"][:, 1])) and np.array_equal(_bits(rf["means"][:, 1]), _bits(rn["means"][:, 1]))


def test_call_with_state_derivatives_keeps_the_first_variant(G):
    """d/dx0 needs every moment of step 1: gpmpc_rollout_jac keeps the full kernel there, on a pack whose rollouts take the new path."""
    cid, N, ds, da = SHAPES[1]
    pb, kinv = OG.problem(cid, N, ds, da, H, B)
    new, old = _pack(G, pb, kinv, NEW), _pack(G, pb, kinv, OLD)
    from gaussian_process_mpc_amd.autograd import RolloutFunction
    rn = _roll(G, new, pb)
    out = []
    for pack in (new, old):
        x0 = torch.tensor(pb["x0"][:B], dtype=torch.float64, device=pack.device, requires_grad=True)
        U = torch.tensor(pb["U"][:B], dtype=torch.float64, device=pack.device)
        means, vars_ = RolloutFunction.apply(x0, U, pack)
        (means[:, 1:].sum() + vars_[:, 1:].sum()).backward()
        out.append({"means": means.detach().cpu().numpy(), "vars": vars_.detach().cpu().numpy(), "dx0": x0.grad.cpu().numpy()})
    jn, jo = out
    _same_bits(jn, jo, "gpmpc_rollout_jac on a pack whose rollouts take the new path")
    np.testing.assert_allclose(jn["means"], rn["means"], rtol=OG.GPU_MEAN_RTOL, atol=1e-9)
    np.testing.assert_allclose(jn["vars"], rn["vars"], rtol=OG.GPU_VAR_RTOL)
    assert np.all(np.isfinite(jn["dx0"])) and np.abs(jn["dx0"]).min() > 0     # the derivatives w.r.t. the state inputs of step 1 are there


def test_step1_quadratic_at_full_size(G):
    """C3 sizes run: N = 2048, ds = 4, da = 1, B = 8, H = 2, path forced, against the old path -- and, where the sum cancels furthest (the
    step-1 weights are formed from M, whose far entries carry the largest relative error), K of step 1 for both paths as in the small cases."""
    from oracle import gpmpc_oracle as O
    from gaussian_process_mpc_amd.synth import synth_problem
    pb = synth_problem(3, 2048, 4, 1, 2, 8)
    kinv = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"]).Ky_inv.numpy()
    cost = G.CostParams(-1.0, pb["Q"], pb["R"])
    res = []
    for env in (NEW, OLD):
        pack = _pack(G, pb, kinv, env)
        _takes(pack, 8, 2, env is NEW)
        res.append(_np(G.rollout(pack, pb["x0"], pb["U"], cost)))
    rn, ro = res
    consts = pack.beta().cpu().numpy().copy(), pack.weights().cpu().numpy()
    kn, amp = _k_step1(pb, consts, (None, None), rn, nb=8)
    ko, _ = _k_step1(pb, consts, (None, None), ro, nb=8)
    print("Q1ACC N=2048 ds=4 da=1 noise=default (B = 8): K_var new %.3g old %.3g | A_var/T up to %.3g" % (kn, ko, amp))
    assert kn <= OG.BUDGET_K["var"] and ko <= OG.BUDGET_K["var"] and kn <= Q1_FACTOR * ko, (kn, ko)
    np.testing.assert_allclose(rn["means"], ro["means"], rtol=OG.GPU_MEAN_RTOL, atol=1e-9)
    np.testing.assert_allclose(rn["vars"], ro["vars"], rtol=OG.GPU_VAR_RTOL)
    np.testing.assert_allclose(rn["cost"], ro["cost"], rtol=OG.GPU_COST_RTOL)
    np.testing.assert_allclose(rn["grad"], ro["grad"], rtol=OG.GPU_GRAD_RTOL, atol=1e-7)
