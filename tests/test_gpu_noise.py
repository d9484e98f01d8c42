"""The noise model of the rollout (gpmpc_pack_set_noise: init_cov, action_var, process_var) through every rollout form, against
tests/noise_reference.py -- the oracle's loops restated over its own single-step functions, pinned to the oracle and shown to move by
>= 10 tolerances under each part alone by tests/test_host_noise.py, on the problems and the model used here:

    ladder problems of tests/offgrid_problems.py (N = 150, H = 3), (ds, da) in {(1, 1), (2, 2), (4, 1), (7, 1)},
    rng = default_rng(5 + ds): init_cov = 0.02 A A^T / ds + diag(U(1e-4, 3e-2)), A ~ U(-1, 1); action_var ~ U(1e-4, 1e-2) with
    action_var[0] = 0 (an exactly known input); process_var ~ U(1e-5, 2e-3)                              (noise_reference.ladder_noise)

Tolerances are the project's (tests/offgrid_problems.py): means 1e-5 (atol 1e-9), variances / covariances 1e-4, cost 1e-6, gradient 1e-4 in
norm and along four directions.  Every reference trajectory is re-asserted sane where it is computed.  Each case asserts from the plan that
the intended form ran.  Without gpmpc_pack_set_noise every test here fails at its first ``set_noise``.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import offgrid_problems as OG
import noise_reference as NR

pytestmark = pytest.mark.gpu

MEAN_RTOL, VAR_RTOL, COST_RTOL, GRAD_RTOL = OG.GPU_MEAN_RTOL, OG.GPU_VAR_RTOL, OG.GPU_COST_RTOL, OG.GPU_GRAD_RTOL
NO_PERSIST = {"GPMPC_PERSIST": "0"}
DIMS = [(1, 1), (2, 2), (4, 1), (7, 1)]
K95 = 1.6448536269514722
_refs, _gps = {}, {}


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


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _np(r):
    return {k: v.detach().cpu().numpy().copy() for k, v in r.items()}


def _pack(G, pb, kinv, **kw):
    return G.GPPack(pb["X"], pb["Y"], kinv, pb["lambdas"], pb["sigma_f"], **kw)


def _cost(G, pb, gamma=-1.0):
    return G.CostParams(gamma, pb["Q"], pb["R"], x_ref=pb["x_ref"], u_ref=pb["u_ref"])


def _gp(args):
    if args not in _gps:
        from oracle import gpmpc_oracle as O
        pb, kinv = OG.problem(*args)
        _gps[args] = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"], Ky_inv=kinv)
    return _gps[args]


def _model(which, ds, da):
    """Keyword arguments of ``set_noise`` / the reference: all three parts of ``ladder_noise`` or one of them alone."""
    P, av, w = NR.ladder_noise(ds, da)
    return {"default": {}, "all": dict(init_cov=P, action_var=av, process_var=w), "init_cov": dict(init_cov=P), "action_var": dict(action_var=av),
            "process_var": dict(process_var=w)}[which]


def _ref(args, gamma, pick, which="all", fullcov=False, nominal=None):
    """Reference trajectories ``pick`` of a problem under a model: computed once per module, sanity re-asserted."""
    pb, _ = OG.problem(*args)
    gp, kw = _gp(args), _model(which, pb["ds"], pb["da"])
    for b in pick:
        key = (args, gamma, which, fullcov, nominal is not None, b)
        if key in _refs:
            continue
        if nominal is not None:
            r = NR.nominal_rollout(gp, nominal[0], nominal[1], pb["H"], pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], gamma, **kw)
        else:
            r = NR.rollout(gp, pb["H"], pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], gamma, fullcov=fullcov, **kw)
        if fullcov:
            OG.assert_fullcov_reference_is_sane(r["means"], r["covs"], r["cost"])
        else:
            OG.assert_diag_reference_is_sane(r["means"], r["vars"], r["cost"], pb["Q"], gamma)
        _refs[key] = r
    keys = ("means", "covs" if fullcov else "vars", "cost", "grad")
    return {k: np.stack([np.asarray(_refs[(args, gamma, which, fullcov, nominal is not None, b)][k]) for b in pick]) for k in keys}


def _excess(a, b, rtol, atol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (atol + rtol * np.abs(b))))


def _assert_grad(got, ref, what):
    """The project's gradient criterion (tests/test_gpu_offgrid.py::_assert_grad): directional derivatives along the reference gradient and
    three seeded directions, 1e-4 relative; and the whole vector in norm."""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    rng = np.random.default_rng(12345)
    dirs = [ref / np.linalg.norm(ref)] + [d / np.linalg.norm(d) for d in rng.standard_normal((3, ref.size))]
    for k, d in enumerate(dirs):
        a, e = float(got @ d), float(ref @ d)
        assert abs(a - e) <= GRAD_RTOL * abs(e), (what, k, a, e)
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    assert err <= GRAD_RTOL, (what, err)
    return err


def _check(r, ref, pick, what, grad=True, fullcov=False):
    """Trajectories ``pick`` of a result against the reference; prints the deviations as fractions of the tolerances before it asserts."""
    r = r if isinstance(r["cost"], np.ndarray) else _np(r)
    assert all(np.all(np.isfinite(v)) for v in r.values()), what
    vk = "covs" if fullcov else "vars"
    atol = 1e-6 * np.abs(ref[vk]).max() if fullcov else 1e-12
    gerr = max(np.linalg.norm(r["grad"][b] - ref["grad"][k]) / np.linalg.norm(ref["grad"][k]) for k, b in enumerate(pick)) if grad else 0.0
    print("DEV %s: means %.3g %s %.3g cost %.3g grad %.3g of the tolerance" % (
        what, _excess(r["means"][pick], ref["means"], MEAN_RTOL, 1e-9), vk, _excess(r[vk][pick], ref[vk], VAR_RTOL, atol),
        _excess(r["cost"][pick], ref["cost"], COST_RTOL, 0.0), gerr / GRAD_RTOL))
    np.testing.assert_allclose(r["means"][pick], ref["means"], rtol=MEAN_RTOL, atol=1e-9, err_msg=what)
    np.testing.assert_allclose(r[vk][pick], ref[vk], rtol=VAR_RTOL, atol=atol, err_msg=what)
    np.testing.assert_allclose(r["cost"][pick], ref["cost"], rtol=COST_RTOL, err_msg=what)
    if grad:
        for k, b in enumerate(pick):
            _assert_grad(r["grad"][b], ref["grad"][k], "%s [%d]" % (what, b))


def _run_diag(G, pack, pb, cost, B, args, gamma, what, which="all", graph=False, nominal=None, pick=None):
    """Objective + gradient and objective only of the first B trajectories under the pack's model, both against the reference."""
    pick = OG.picks(B) if pick is None else pick
    ref = _ref(args, gamma, pick, which, nominal=nominal)
    r = _np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, graph=graph))
    f = _np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=False, graph=graph))
    _check(r, ref, pick, what)
    _check(f, ref, pick, what + " objective only", grad=False)
    return r


def _run_fullcov(G, pack, pb, cost, B, args, what, which="all"):
    pick = OG.picks(B)
    ref = _ref(args, -1.0, pick, which, fullcov=True)
    r = _np(G.rollout_fullcov(pack, pb["x0"][:B], pb["U"][:B], cost))
    f = _np(G.rollout_fullcov(pack, pb["x0"][:B], pb["U"][:B], cost, want_grad=False))
    _check(r, ref, pick, what, fullcov=True)
    _check(f, ref, pick, what + " objective only", grad=False, fullcov=True)
    return r


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the form ladder under the model
# ------------------------------------------------------------------------------------------------------------------------------
LADDER_EXPECTED = {("fused_staged", "64x64", "quarter columns"), ("fused_staged", "64x64", "whole tiles"), ("head+pair_sb", "256x64", "tb1"),
                   ("fused_sb", "256x64", ""), ("fused_sb", "256x32", ""), ("fused_sb", "256x16", ""), ("persist", "", "16 waves"),
                   ("persist", "", "8 waves"), ("head+pair_sb", "256x256", "big"), ("head+pair_staged", "64x64", "")}


@pytest.mark.parametrize("ds,da", DIMS)
def test_form_ladder_under_the_model(G, ds, da):
    """The steps of tests/test_gpu_offgrid.py::test_diag_form_ladder_vs_cport with all three parts of the model set: each form asserted from
    the plan, the set reached the whole set; objective + gradient and objective only; one captured graph per dimension; step 0 exact."""
    D = ds + da
    bs = OG.ladder_batches(ds)
    args = (OG.ladder_config(ds, da), OG.LADDER_N, ds, da, OG.LADDER_H, bs["big"], False)
    pb, kinv = OG.problem(*args)
    H = pb["H"]
    pack, cost = _pack(G, pb, kinv), _cost(G, pb)
    kw = _model("all", ds, da)
    pack.set_noise(**kw)
    assert not pack.noise_is_default
    for got, want in zip(pack.noise, (kw["init_cov"], kw["action_var"], kw["process_var"])):
        np.testing.assert_array_equal(got, want)
    narrow = {"GPMPC_FUSED_SB": "1", "GPMPC_PAIR_SB": "1"}
    steps = [(bs["small"],       {},                                         "fused_staged",     "64x64",   "quarter columns", ",4,1>"),
             (bs["one"],         {},                                         "fused_staged",     "64x64",   "quarter columns", ",4,1>"),
             (bs["whole_tiles"], {},                                         "fused_staged",     "64x64",   "whole tiles",     ",1,1>"),
             (bs["mid"],         NO_PERSIST,                                 "head+pair_sb",     "256x64",  "tb1",             ""),
             (bs["mid"],         {"GPMPC_FUSED_SB": "1"},                    "fused_sb",         "256x64",  "",                ",0,1>"),
             (5,                 dict(narrow, GPMPC_TILING="5"),             "fused_sb",         "256x32",  "",                ",32,1>"),
             (4,                 dict(narrow, GPMPC_TILING="6"),             "fused_sb",         "256x16",  "",                ",16,1>"),
             (7,                 {"GPMPC_PERSIST": "16"},                    "persist",          "",        "16 waves",        "x16waves"),
             (6,                 {"GPMPC_PERSIST": "8"},                     "persist",          "",        "8 waves",         "x8waves"),
             (bs["big"],         NO_PERSIST,                                 "head+pair_sb",     "256x256", "big",             ""),
             (5,                 {"GPMPC_PAIR_SB": "0", "GPMPC_FUSED": "0"}, "head+pair_staged", "64x64",   "",                "")]
    reached = set()
    for B, env, form, tiling, tag, kern in steps:
        with _tuning(pack, env):
            plan = pack.plan(B, H)
            assert plan["form"] == form and (not tiling or plan["tiling"] == tiling) and kern in plan["kernel"], (B, env, plan)
            if tag == "big":
                assert plan["tb"] == (2 if D <= 5 else 1) and B % 2 == 1, plan
            if tag == "tb1":
                assert plan["tb"] == 1, plan
            assert pack.plan(B, H, want_grad=False)["form"] == form
            what = "noise ds=%d da=%d B=%d %s %s %s" % (ds, da, B, form, tiling, tag)
            r = _run_diag(G, pack, pb, cost, B, args, -1.0, what)
            np.testing.assert_array_equal(_bits(r["vars"][:, 0, :]), _bits(np.tile(np.diag(kw["init_cov"]), (B, 1))), err_msg=what)      # step 0
            if tag == "tb1":
                gplan = pack.plan(B, H, graph=True)
                assert gplan["form"] == form and gplan["tiling"] == tiling, gplan
                _run_diag(G, pack, pb, cost, B, args, -1.0, what + " graph split=%d" % gplan["split"], graph=True)
        reached.add((form, tiling, tag))
    assert reached == LADDER_EXPECTED, reached ^ LADDER_EXPECTED
    assert not pack.noise_is_default                       # (reload_tuning keeps the model)


def test_shared_lambda_forms_under_the_model(G):
    """The other kernel copies a shared-lambda pack takes (tests/test_gpu_offgrid.py, SHARED_DIMS[1]: one group of three GPs): head+pair_sbs,
    the shared one-launch form, the whole-horizon kernel over one unit of all GPs."""
    ds, da = OG.SHARED_DIMS[1]
    bs = OG.shared_batches(ds)
    args = (OG.shared_config(ds, da), OG.LADDER_N, ds, da, OG.LADDER_H, max(bs.values()), True)
    pb, kinv = OG.problem(*args)
    H = pb["H"]
    pack, cost = _pack(G, pb, kinv), _cost(G, pb)
    assert pack.shared_lambda
    pack.set_noise(**_model("all", ds, da))
    steps = [(bs["mid"],     NO_PERSIST,               "head+pair_sbs",   "256x64", ",3,%d," % ds),
             (bs["mid"],     {"GPMPC_FUSED_SB": "1"},  "fused_sb_shared", "256x64", ",0,3>"),
             (bs["persist"], {"GPMPC_PERSIST": "16"},  "persist",         "",       ",%d>x16waves" % ds)]
    for B, env, form, tiling, kern in steps:
        with _tuning(pack, env):
            plan = pack.plan(B, H)
            assert plan["form"] == form and (not tiling or plan["tiling"] == tiling) and kern in plan["kernel"].replace(" ", ""), (B, env, plan)
            _run_diag(G, pack, pb, cost, B, args, -1.0, "noise shared ds=%d B=%d %s" % (ds, B, form))


@pytest.mark.parametrize("ng", [2, 4])
def test_spilling_one_launch_instances_at_ds7_with_one_lambda(G, ng):
    """k_step_fused<8, 7, *, 0, 2> and <8, 7, *, 0, 4>: the shared one-launch form of a ds = 7, da = 1 pack in groups of two and of four GPs
    (GPMPC_SHARED_NG at pack creation; the planner's own choice is three), instances that spill VGPRs within the spill guard's exemption.
    Whatever carries process_var to the store of sp[2] has to survive those spills: at the defaults (w = 0, where a lost value shows as
    garbage in every variance) and under the model, objective + gradient and objective only, against the reference."""
    ds, da = 7, 1
    B = 2048 // (3 * ds) + 2
    args = (OG.shared_config(ds, da), OG.LADDER_N, ds, da, OG.LADDER_H, B, True)
    pb, kinv = OG.problem(*args)
    H = pb["H"]
    old = os.environ.get("GPMPC_SHARED_NG")
    os.environ["GPMPC_SHARED_NG"] = str(ng)
    try:
        pack = _pack(G, pb, kinv)
    finally:
        if old is None:
            os.environ.pop("GPMPC_SHARED_NG", None)
        else:
            os.environ["GPMPC_SHARED_NG"] = old
    cost = _cost(G, pb)
    assert pack.shared_lambda
    with _tuning(pack, {"GPMPC_FUSED_SB": "1"}):
        for want_grad in (True, False):
            plan = pack.plan(B, H, want_grad=want_grad)
            assert plan["form"] == "fused_sb_shared" and plan["tiling"] == "256x64", plan
            assert ("k_step_fused<8,7,%s,0,%d>" % ("true" if want_grad else "false", ng)) in plan["kernel"].replace(" ", ""), plan
        for which in ("default", "all"):
            pack.set_noise(**_model(which, ds, da))
            _run_diag(G, pack, pb, cost, B, args, -1.0, "noise shared ds=7 groups of %d, %s model, B=%d" % (ng, which, B), which=which)


def test_nominal_pack_under_the_model(G):
    """Case "c3" of tests/test_gpu_offgrid.py's nominal packs (N = 449, ds = 4, H = 10), B = 1 and 64: the nominal twins of the head kernel
    read the same buffer (action_var also enters their linear terms n_k^2 s_k)."""
    from nominal_reference import synth_nominal
    cfg, N, ds, da, H, shared, gamma = OG.DIAG_CASES[2]
    args = (cfg, N, ds, da, H, 64, shared)
    pb, kinv = OG.problem(*args)
    nominal = synth_nominal(ds, da)
    pack, cost = _pack(G, pb, kinv, nominal=nominal), _cost(G, pb, gamma)
    pack.set_noise(**_model("all", ds, da))
    for B in (1, 64):
        plan = pack.plan(B, H)
        assert plan.get("nominal") == 1 and plan["launches_per_step"] == 2, plan
        _run_diag(G, pack, pb, cost, B, args, gamma, "noise nominal c3 B=%d %s" % (B, plan["form"]), nominal=nominal, pick=sorted({0, B - 1}))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. full covariance
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", OG.FULLCOV_CASES[:2], ids=lambda c: "ds%d-da%d-N%d%s" % (c[2], c[3], c[1], "-shared" if c[4] else ""))
def test_fullcov_under_the_model(G, case):
    """FULLCOV_CASES' smallest case and its ds = 3 case (one lambda): two-launch at B = 1 and 3, four-launch at B = 3 and the large-batch
    kernel's batch, the cross-unit kernel at B = 3.  Means, whole covariances, cost, gradient; an off-diagonal init_cov shows in covs[:, 1]."""
    cfg, N, ds, da, shared = case
    H, b_big = OG.FULLCOV_H, OG.fullcov_big_batch(ds)
    args = (cfg, N, ds, da, H, b_big, shared)
    pb, kinv = OG.problem(*args)
    pack, cost = _pack(G, pb, kinv), _cost(G, pb)
    pack.enable_fullcov()
    kw = _model("all", ds, da)
    pack.set_noise(**kw)
    cases = [(1, {"GPMPC_FC_FORM": "1"}, "two_launch"), (3, {"GPMPC_FC_FORM": "1"}, "two_launch"),
             (3, {"GPMPC_FC_FORM": "0"}, "four_launch"), (b_big, {"GPMPC_FC_FORM": "0"}, "four_launch")]
    if shared:
        assert pack.shared_lambda
        cases.append((3, {"GPMPC_FC_SHARED": "1"}, "two_launch"))
    # the reference itself: the off-diagonal of init_cov reaches the covariance of step 1
    diag_only = NR.rollout(_gp(args), H, pb["x0"][0], pb["U"][0], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], -1.0, fullcov=True,
                           **dict(kw, init_cov=np.diag(np.diag(kw["init_cov"]))))
    full = _ref(args, -1.0, [0], fullcov=True)
    assert _excess(full["covs"][0][1], diag_only["covs"][1], VAR_RTOL, 1e-6 * np.abs(full["covs"]).max()) >= 10.0
    for B, env, form in cases:
        what = "noise fullcov ds=%d da=%d N=%d B=%d %s" % (ds, da, N, B, env)
        with _tuning(pack, env):
            plan = pack.plan_fullcov(B, H)
            assert plan["form"] == form, (env, plan)
            if "GPMPC_FC_SHARED" in env:
                assert plan["shared_cross_units"] == 1, plan
            r = _run_fullcov(G, pack, pb, cost, B, args, what)
        np.testing.assert_array_equal(_bits(r["covs"][:, 0]), _bits(np.tile(kw["init_cov"], (B, 1, 1))), err_msg=what)      # step 0: the whole matrix


# ------------------------------------------------------------------------------------------------------------------------------
# 3. / 4. / 5. the defaults are inert; each part reaches each family; step 0
# ------------------------------------------------------------------------------------------------------------------------------
FAMILIES = [("two_launch", 5, {"GPMPC_PAIR_SB": "0", "GPMPC_FUSED": "0"}, "head+pair_staged"), ("fused", 3, {}, "fused_staged"),
            ("persist", 7, {"GPMPC_PERSIST": "16"}, "persist")]
FC_FORMS = [("fc_two", 3, {"GPMPC_FC_FORM": "1"}, "two_launch"), ("fc_four", 3, {"GPMPC_FC_FORM": "0"}, "four_launch")]


def _ladder22(G):
    ds, da = 2, 2
    args = (OG.ladder_config(ds, da), OG.LADDER_N, ds, da, OG.LADDER_H, OG.ladder_batches(ds)["big"], False)
    pb, kinv = OG.problem(*args)
    return args, pb, kinv


def test_defaults_set_explicitly_are_inert(G):
    """A pack with the defaults SET equals a pack never touched, bit for bit, in every output of one case per form family; get says 0.
    (With w = 0 the sum sf^2 + w is sf^2 exactly, and the uploaded constants are the ones the kernels used to carry.)"""
    args, pb, kinv = _ladder22(G)
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    cost = _cost(G, pb)
    plain, touched = _pack(G, pb, kinv).enable_fullcov(), _pack(G, pb, kinv).enable_fullcov()
    P, av, w = NR.defaults(ds, da)
    touched.set_noise(init_cov=P, action_var=av, process_var=w)
    assert touched.noise_is_default and plain.noise_is_default
    for got, want in zip(plain.noise, (P, av, w)):
        np.testing.assert_array_equal(_bits(got), _bits(want))
    for tag, B, env, form in FAMILIES + FC_FORMS:
        out = []
        for pack in (plain, touched):
            with _tuning(pack, env):
                if tag.startswith("fc"):
                    assert pack.plan_fullcov(B, H)["form"] == form
                    out.append(_np(G.rollout_fullcov(pack, pb["x0"][:B], pb["U"][:B], cost)))
                else:
                    assert pack.plan(B, H)["form"] == form
                    out.append(_np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost)))
        for k in out[0]:
            np.testing.assert_array_equal(_bits(out[0][k]), _bits(out[1][k]), err_msg="%s %s" % (tag, k))
    # ... and a model that was set and then cleared
    touched.set_noise(**_model("all", ds, da))
    assert not touched.noise_is_default
    touched.set_noise()
    assert touched.noise_is_default
    a, b = _np(G.rollout(plain, pb["x0"][:3], pb["U"][:3], cost)), _np(G.rollout(touched, pb["x0"][:3], pb["U"][:3], cost))
    for k in a:
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg="cleared " + k)


@pytest.mark.parametrize("which", ["init_cov", "action_var", "process_var"])
def test_each_part_alone_reaches_each_family(G, which):
    """Only one part set (the others at their defaults), on one two-launch, one one-launch, one whole-horizon and both full-covariance cases,
    against the reference under that part alone: tests/test_host_noise.py shows that ignoring the part misses a tolerance by a factor >= 10
    on this very problem."""
    args, pb, kinv = _ladder22(G)
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    pack, cost = _pack(G, pb, kinv).enable_fullcov(), _cost(G, pb)
    kw = _model(which, ds, da)
    pack.set_noise(**kw)
    P0, av0, w0 = NR.defaults(ds, da)
    P, av, w = pack.noise
    np.testing.assert_array_equal(P, kw.get("init_cov", P0))
    np.testing.assert_array_equal(av, kw.get("action_var", av0))
    np.testing.assert_array_equal(w, kw.get("process_var", w0))
    for tag, B, env, form in FAMILIES + FC_FORMS:
        what = "noise only %s: %s B=%d" % (which, tag, B)
        with _tuning(pack, env):
            if tag.startswith("fc"):
                assert pack.plan_fullcov(B, H)["form"] == form
                r = _run_fullcov(G, pack, pb, cost, B, args, what, which=which)
                np.testing.assert_array_equal(_bits(r["covs"][:, 0]), _bits(np.tile(P, (B, 1, 1))), err_msg=what)
            else:
                assert pack.plan(B, H)["form"] == form
                r = _run_diag(G, pack, pb, cost, B, args, -1.0, what, which=which)
                np.testing.assert_array_equal(_bits(r["vars"][:, 0, :]), _bits(np.tile(np.diag(P), (B, 1))), err_msg=what)


# ------------------------------------------------------------------------------------------------------------------------------
# 6. graph replay follows the values
# ------------------------------------------------------------------------------------------------------------------------------
def test_one_captured_callback_graph_follows_a_new_init_cov_per_solve(G):
    """The estimator-driven loop: a different init_cov before each of 5 solver callbacks.  One capture serves all of them; each result is
    the eager rollout under the same values bit for bit, and differs from the one before."""
    from gaussian_process_mpc_amd._lib import lib
    args, pb, kinv = _ladder22(G)
    ds, da = pb["ds"], pb["da"]
    pack, cost = _pack(G, pb, kinv), _cost(G, pb)
    P, av, w = NR.ladder_noise(ds, da)
    prev = None
    for k in range(5):
        pack.set_noise(init_cov=(1.0 + 0.5 * k) * P, action_var=av, process_var=w)
        cg = pack.objective_gradient(pb["x0"][0], pb["U"][0], cost).copy()
        eager = _np(G.rollout(pack, pb["x0"][0], pb["U"][0], cost, want_traj=False))
        np.testing.assert_array_equal(_bits(cg[:1]), _bits(eager["cost"]))
        np.testing.assert_array_equal(_bits(cg[1:]), _bits(eager["grad"].reshape(-1)))
        if prev is not None:
            assert cg[0] != prev[0] and not np.array_equal(cg[1:], prev[1:])
        prev = cg
    assert lib().gpmpc_pack_callback_captures(pack.handle) == 1
    ref = NR.rollout(_gp(args), pb["H"], pb["x0"][0], pb["U"][0], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], -1.0, init_cov=3.0 * P, action_var=av,
                     process_var=w)
    np.testing.assert_allclose(prev[0], ref["cost"], rtol=COST_RTOL)          # (the last one against the reference under ITS values)
    _assert_grad(prev[1:], ref["grad"], "callback under 3 P")
    # the batched graph too: replayed under new values without a new capture
    r0 = _np(G.rollout(pack, pb["x0"][:3], pb["U"][:3], cost, graph=True))
    n0 = lib().gpmpc_pack_graph_captures(pack.handle)
    pack.set_noise(init_cov=P, action_var=av, process_var=w)
    r1 = _np(G.rollout(pack, pb["x0"][:3], pb["U"][:3], cost, graph=True))
    e1 = _np(G.rollout(pack, pb["x0"][:3], pb["U"][:3], cost))
    assert lib().gpmpc_pack_graph_captures(pack.handle) == n0
    for key in ("cost", "grad", "means", "vars"):
        np.testing.assert_array_equal(_bits(r1[key]), _bits(e1[key]), err_msg=key)
    assert not np.array_equal(r0["cost"], r1["cost"])


# ------------------------------------------------------------------------------------------------------------------------------
# 7. consumers: chance constraints and the device solvers
# ------------------------------------------------------------------------------------------------------------------------------
def _c1():
    """The c1 constraint problem of tests/test_gpu_constraints.py: synth_problem(1, 100, 2, 2, 10, 64), gamma = 1e-5, its three rows."""
    if "c1" not in _gps:
        from gaussian_process_mpc_amd.synth import synth_problem
        from oracle import gpmpc_oracle as O
        pb = synth_problem(1, 100, 2, 2, 10, 64)
        gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"])
        rng = np.random.default_rng(77 + pb["ds"])
        A = rng.standard_normal((3, pb["ds"]))
        A[0] = 0.0
        A[0, 0] = 1.0
        _gps["c1"] = (pb, gp, (A, np.array([0.5, 0.2, 0.1]), np.array([K95, 2.0, 0.0])))
    return _gps["c1"]


def test_constraints_follow_the_model(G):
    """g and its dense Jacobian from gpmpc_rollout_constrained under the model, against the DEFINITION of the rows
    (tests/constraints_reference.py::g_of_trajectory) applied to the noise reference's trajectory, Jacobian by autograd row by row;
    tolerances of tests/test_gpu_constraints.py.  The model moves g by far more than they allow."""
    from constraints_reference import g_of_trajectory
    pb, gp, (A, bb, kap) = _c1()
    ds, da, H, gamma = pb["ds"], pb["da"], pb["H"], 1e-5
    kw = _model("all", ds, da)
    pack = G.GPPack(pb["X"], pb["Y"], gp.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"])
    sc, cost = G.StateConstraints(A, bb, kappa=kap), G.CostParams(gamma, pb["Q"], pb["R"], x_ref=pb["x_ref"], u_ref=pb["u_ref"])
    B, b = 2, 1
    plain = _np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, constraints=sc))
    pack.set_noise(**kw)
    one = _np(G.rollout(pack, pb["x0"][:B], pb["U"][:B], cost, constraints=sc))
    Ut = torch.as_tensor(pb["U"][b].copy()).reshape(H, da).requires_grad_(True)
    means, vars_ = NR.trajectory(gp, H, pb["x0"][b], Ut, **kw)
    g = g_of_trajectory(means, vars_, A, bb, kap)
    m_c = g.shape[1]
    jac = np.stack([torch.autograd.grad(g[t, r], Ut, retain_graph=True)[0].reshape(-1).numpy() for t in range(H) for r in range(m_c)])
    mu, var = torch.stack([m.detach() for m in means]).numpy(), torch.stack([v.detach() for v in vars_]).numpy()
    OG.assert_diag_reference_is_sane(mu, var, 0.0, pb["Q"], gamma)
    sd = np.sqrt(np.stack([(A ** 2) @ v for v in var[1:]]))
    tol = 1e-5 * (np.abs(mu[1:, None, :] * A[None, :, :])).sum(axis=2) + 0.5e-4 * kap[None, :] * sd + 1e-9
    err = np.abs(one["g"][b] - g.detach().numpy())
    print("DEV noise constraints: g %.3g of the tolerance; the model moves g by %.3g tolerances" % ((err / tol).max(), (np.abs(plain["g"][b] - one["g"][b]) / tol).max()))
    assert np.all(err <= tol), err.max()
    assert (np.abs(plain["g"][b] - one["g"][b]) / tol).max() >= 10.0
    for i in range(H * m_c):
        _assert_grad(one["g_jac"][b][i], jac[i], "noise constraints row %d" % i)
    _assert_grad(one["g_jac"][b], jac, "noise constraints whole matrix")
    np.testing.assert_allclose(one["means"][b], mu, rtol=MEAN_RTOL, atol=1e-9)
    np.testing.assert_allclose(one["vars"][b], var, rtol=VAR_RTOL, atol=1e-12)


def test_device_solvers_follow_the_model(G):
    """solver "mppi", "lbfgs" and "auglag" call gpmpc_enqueue_rollout on the pack: under the model, the cost each reports for a plan is the
    cost ONE rollout of the same pack gives that plan in a call of the solver's shape, bit for bit -- and not the cost under the defaults.
    Small K, few iterations: this is about which numbers the solvers see, not about how well they solve."""
    from gaussian_process_mpc_amd.mppi import mppi_solve
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_solve
    from gaussian_process_mpc_amd.device_auglag import auglag_solve
    pb, gp, (A, bb, kap) = _c1()
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    pack = G.GPPack(pb["X"], pb["Y"], gp.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"])
    cost = G.CostParams(1e-5, pb["Q"], pb["R"], x_ref=pb["x_ref"], u_ref=pb["u_ref"])
    sc = G.StateConstraints(A[:1], [0.45], kappa=[K95])
    kw = _model("all", ds, da)
    x0, K = pb["x0"][0], 4
    lb, ub = -np.ones(da), np.ones(da)
    X0 = np.random.default_rng(11).uniform(-0.5, 0.5, (K, H, da))
    X0[0] = 0.0

    def again(plans, grad, cons):
        r = G.rollout(pack, x0, plans, cost, want_grad=grad, want_traj=False, constraints=cons)
        return r["cost"].cpu().numpy()

    pack.set_noise(**kw)
    m = mppi_solve(pack, x0, np.zeros((H, da)), cost, constraints=sc, samples=16, iterations=3, sigma=0.3, seed=5, lb=lb, ub=ub)
    c_m = again(np.tile(m["U"], (16, 1, 1)), False, sc)
    assert _bits(c_m[:1])[0] == _bits(np.array([m["cost"]]))[0], (c_m[0], m["cost"])
    _, _, li = lbfgs_solve(pack, x0, X0, cost, lb=lb, ub=ub, max_ticks=6, check_every=3)
    c_l = again(li["x"].reshape(K, H, da), True, None)
    np.testing.assert_array_equal(_bits(c_l), _bits(li["f"]))
    Ua, fa, ai = auglag_solve(pack, x0, X0, cost, sc, lb=lb, ub=ub, outer=2, inner_ticks=4)
    c_a = again(np.asarray(ai["x"]).reshape(K, H, da), True, sc)
    np.testing.assert_array_equal(_bits(c_a), _bits(np.asarray(ai["f"])))
    # the same plans under the defaults cost something else: the solvers did see the model
    pack.set_noise()
    for plans, grad, cons, seen in ((np.tile(m["U"], (16, 1, 1)), False, sc, c_m), (li["x"].reshape(K, H, da), True, None, c_l),
                                    (np.asarray(ai["x"]).reshape(K, H, da), True, sc, c_a)):
        d = again(plans, grad, cons)
        assert np.all(np.abs(d - seen) > 100 * COST_RTOL * np.abs(seen)), (d, seen)


# ------------------------------------------------------------------------------------------------------------------------------
# 8. life cycle
# ------------------------------------------------------------------------------------------------------------------------------
def test_model_survives_resize_and_is_cleared_by_all_none(G):
    args, pb, kinv = _ladder22(G)
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    pack, cost = _pack(G, pb, kinv), _cost(G, pb)
    kw = _model("all", ds, da)
    pack.set_noise(**kw)
    before = _np(G.rollout(pack, pb["x0"][:3], pb["U"][:3], cost))
    # a smaller training set of the same padded size: gpmpc_pack_resize + a build, then back
    from oracle import gpmpc_oracle as O
    n = OG.LADDER_N - 7
    small = O.GPBundle(pb["X"][:n], pb["Y"][:n], pb["lambdas"], pb["sigma_f"], pb["sigma_n"])
    h = pack.handle
    assert pack.rebuild(pb["X"][:n], pb["Y"][:n], small.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"]) and pack.handle is h and pack.N == n
    assert not pack.noise_is_default
    for got, want in zip(pack.noise, (kw["init_cov"], kw["action_var"], kw["process_var"])):
        np.testing.assert_array_equal(got, want)
    mid = _np(G.rollout(pack, pb["x0"][:3], pb["U"][:3], cost))
    np.testing.assert_array_equal(_bits(mid["vars"][:, 0, :]), _bits(np.tile(np.diag(kw["init_cov"]), (3, 1))))
    for b in (0, 2):
        r = NR.rollout(small, H, pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], -1.0, **kw)
        OG.assert_diag_reference_is_sane(r["means"], r["vars"], r["cost"], pb["Q"], -1.0)
        np.testing.assert_allclose(mid["vars"][b], r["vars"], rtol=VAR_RTOL, atol=1e-12)
        np.testing.assert_allclose(mid["cost"][b], r["cost"], rtol=COST_RTOL)
    assert pack.rebuild(pb["X"], pb["Y"], kinv, pb["lambdas"], pb["sigma_f"]) and pack.handle is h
    after = _np(G.rollout(pack, pb["x0"][:3], pb["U"][:3], cost))
    for k in before:
        np.testing.assert_array_equal(_bits(before[k]), _bits(after[k]), err_msg=k)
    pack.set_noise()
    assert pack.noise_is_default
    fresh = _np(G.rollout(_pack(G, pb, kinv), pb["x0"][:3], pb["U"][:3], cost))
    cleared = _np(G.rollout(pack, pb["x0"][:3], pb["U"][:3], cost))
    for k in fresh:
        np.testing.assert_array_equal(_bits(fresh[k]), _bits(cleared[k]), err_msg=k)
    # refused values leave the pack as it was
    pack.set_noise(**kw)
    for bad in (dict(init_cov=-kw["init_cov"]), dict(action_var=[float("nan")] * da), dict(process_var=[-1.0] * ds),
                dict(init_cov=kw["init_cov"] + np.triu(np.full((ds, ds), 1e-6), 1))):
        with pytest.raises(G.GpmpcError):
            pack.set_noise(**bad)
        for got, want in zip(pack.noise, (kw["init_cov"], kw["action_var"], kw["process_var"])):
            np.testing.assert_array_equal(got, want)
    again = _np(G.rollout(pack, pb["x0"][:3], pb["U"][:3], cost))
    np.testing.assert_array_equal(_bits(again["cost"]), _bits(before["cost"]))


def test_dynamics_and_mpc_keep_the_model_across_a_new_pack(G):
    """Dynamics stores the model and re-applies it when appends outgrow the padded size (a NEW pack); "sigma_n" follows the GPs' noise;
    RiskSensitiveMPC's callbacks, batched evaluation and full-covariance path follow; set_initial_covariance changes init_cov alone."""
    args, pb, kinv = _ladder22(G)
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    P, av, w = NR.ladder_noise(ds, da)
    mpc = G.RiskSensitiveMPC(-1.0, H, ds, da, pb["Q"], pb["R"])
    for a, g in enumerate(mpc.dynamics.gpr_err):
        g.set_lambdas(pb["lambdas"][a])
        g.set_sigma_n(np.array(pb["sigma_n"][a]))
        g.set_sigma_f(np.array(pb["sigma_f"][a]))
    n0 = 120                                                   # pads to 128: 30 more rows need a new pack (150 -> 192)
    dyn = mpc.dynamics
    dyn.append_train_data(pb["X"][:n0, :ds], pb["X"][:n0, ds:], pb["Y"][:n0])
    mpc.set_xref(pb["x_ref"])
    mpc.set_uref(pb["u_ref"])
    mpc.set_noise_model(init_cov=P, action_var=av, process_var="sigma_n")
    first = dyn.pack()
    sn2 = np.array([float(g.get_sigma_n()) ** 2 for g in dyn.gpr_err])
    np.testing.assert_array_equal(first.noise[0], P)
    np.testing.assert_array_equal(first.noise[2], sn2)
    dyn.append_train_data(pb["X"][n0:, :ds], pb["X"][n0:, ds:], pb["Y"][n0:])
    second = dyn.pack()
    assert second is not first and second.Np == 192
    for got, want in zip(second.noise, (P, av, sn2)):
        np.testing.assert_array_equal(got, want)
    from oracle import gpmpc_oracle as O
    Kinv = torch.stack([g.Ky_inv.detach().cpu() for g in dyn.gpr_err])
    gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"], Ky_inv=Kinv)
    x0, U = pb["x0"][0], pb["U"][0]

    def callbacks():
        mpc.curr_state = torch.tensor(x0, dtype=torch.float64, device=mpc.device)
        mpc._cache_key = None
        x = U.reshape(-1).copy()
        return mpc.objective(x), np.asarray(mpc.gradient(x)).reshape(-1)

    ref = NR.rollout(gp, H, x0, U, pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], -1.0, init_cov=P, action_var=av, process_var=sn2)
    OG.assert_diag_reference_is_sane(ref["means"], ref["vars"], ref["cost"], pb["Q"], -1.0)
    c, g = callbacks()
    np.testing.assert_allclose(c, ref["cost"], rtol=COST_RTOL)
    _assert_grad(g, ref["grad"], "class path callbacks")
    r = _np(mpc.evaluate_batch(torch.as_tensor(pb["U"][:1], device=mpc.device), curr_state=torch.as_tensor(pb["x0"][:1], device=mpc.device)))
    _check(r, {k: np.asarray(ref[k])[None] for k in ("means", "vars", "cost", "grad")}, [0], "class path evaluate_batch")
    mv, cv = dyn.forward_propagate_torch(H, x0, U)
    np.testing.assert_allclose(torch.stack([torch.diagonal(s) for s in cv]).cpu().numpy(), ref["vars"], rtol=VAR_RTOL, atol=1e-12)
    # a new sigma_n is followed (the GPs rebuild, the pack is refilled, process_var is set again)
    for gq in dyn.gpr_err:
        gq.set_sigma_n(np.array(0.05))
        gq.build_Ky_inv_mat()
    np.testing.assert_array_equal(dyn.pack().noise[2], np.full(ds, float(dyn.gpr_err[0].get_sigma_n()) ** 2))
    # the per-solve call: init_cov alone changes
    mpc.set_initial_covariance(2.0 * P)
    got = dyn.pack().noise
    np.testing.assert_array_equal(got[0], 2.0 * P)
    np.testing.assert_array_equal(got[1], av)
    # full covariance honours the whole matrix
    mpc.full_covariance = True
    mpc.set_noise_model(init_cov=P, action_var=av, process_var=w)
    Kinv = torch.stack([g.Ky_inv.detach().cpu() for g in dyn.gpr_err])
    gp2 = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], [0.05] * ds, Ky_inv=Kinv)
    reff = NR.rollout(gp2, H, x0, U, pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], -1.0, init_cov=P, action_var=av, process_var=w, fullcov=True)
    OG.assert_fullcov_reference_is_sane(reff["means"], reff["covs"], reff["cost"])
    c, g = callbacks()
    np.testing.assert_allclose(c, reff["cost"], rtol=COST_RTOL)
    _assert_grad(g, reff["grad"], "class path, full covariance")
    mpc.set_noise_model()
    assert dyn.pack().noise_is_default
