"""Rollout problems OFF the grid every other rollout test sits on (sigma_f = 1 for every GP, x_ref = u_ref = 0, diagonal Q): the inputs of
tests/test_host_offgrid.py (which pins the C ports to the torch oracle on them) and tests/test_gpu_offgrid.py (which holds every rollout
kernel form to the C ports on them, asserting from the plan that each batch size tabulated below reaches the form it is meant for).  A plain helper module: no fixtures, no collection hooks.

``offgrid(pb, seed)`` takes a ``synth_problem`` dict and draws, in this order, from ``np.random.default_rng(seed)``:

    sigma_f = U(0.6, 1.8) per GP (distinct)      x_ref = U(-0.5, 0.5)      u_ref = U(-0.3, 0.3)      Q += 0.02 (ones - eye)

The amplitude enters each kernel form in its own code (folded pair weights sf^4, the mean factor sf^2 / sqrt(det), var = sf^2 - T - mu^2,
the cross-unit weights sf_a^2 sf_b^2, groups of GPs that share one exponent but not one amplitude): every factor is 1 on the grid.
``Ky_inv`` always comes from ``oracle.GPBundle`` built with the new amplitudes.
"""
import numpy as np

SIGMA_F_RANGE = (0.6, 1.8)

# the project's tolerances on the GPU (tests/test_gpu_instances.py): means, variances / covariances, cost, gradient
GPU_MEAN_RTOL, GPU_VAR_RTOL, GPU_COST_RTOL, GPU_GRAD_RTOL = 1e-5, 1e-4, 1e-6, 1e-4

#                config N    ds da H   shared gamma
DIAG_CASES = [(1,     100, 2, 2, 10, False, 1e-5),
              (2,     200, 3, 1, 20, False, -1.0),
              (3,     449, 4, 1, 10, False, -1.0),
              (3,     449, 4, 1, 10, True,  -1.0),
              (4,     300, 6, 1, 6,  False, -1.0),
              (3,     130, 1, 1, 6,  False, -1.0),
              (5,     320, 5, 2, 5,  False, -1.0),
              (7,     260, 7, 1, 4,  False, -1.0)]
#                config N    ds da shared         (H = 3, B = 2, gamma = -1)
FULLCOV_CASES = [(11,   110, 2, 1, False),
                 (12,   130, 3, 2, True),
                 (13,   300, 4, 2, False),
                 (14,   110, 5, 1, True),
                 (15,   150, 6, 1, False)]
FULLCOV_H, FULLCOV_B = 3, 2


# The rounding-error budget (tests/test_gpu_accuracy.py, tests/test_host_accuracy.py): K = max |error| / (2^-53 x sum of absolute terms) per step.
# One number per quantity for all forms: twice the worst K measured on an MI355X (means 0.88, variances 0.342, covariances 0.30; the table in
# tests/test_gpu_accuracy.py), rounded up to one significant digit.  Whole trajectory, against the long double complex step: relative error
# of the cost (worst 9.5e-10) and of the gradient in norm (worst 7.4e-10), both at N = 520, the worst-conditioned problem of the tables.
BUDGET_K = {"mean": 2.0, "var": 0.7, "cov": 0.6}
BUDGET_TRAJ = {"cost": 2e-9, "grad": 2e-9}
EXCESS_FACTOR = 10.0                                     # a form further than this above K_ref (the floor) on the same case is traced, not absorbed


def seed_of(config_id):
    return 77 + config_id


def offgrid(pb, seed):
    """Move a ``synth_problem`` dict off the grid, in place (and return it)."""
    rng = np.random.default_rng(seed)
    ds, da = pb["ds"], pb["da"]
    pb["sigma_f"] = rng.uniform(SIGMA_F_RANGE[0], SIGMA_F_RANGE[1], ds)
    pb["x_ref"] = rng.uniform(-0.5, 0.5, ds)
    pb["u_ref"] = rng.uniform(-0.3, 0.3, da)
    pb["Q"] = pb["Q"] + 0.02 * (np.ones((ds, ds)) - np.eye(ds))
    return pb


def bundle(pb, sigma_f=None):
    """``oracle.GPBundle`` of a problem (Ky_inv from its amplitudes, or from ``sigma_f`` given instead)."""
    from oracle import gpmpc_oracle as O
    return O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"] if sigma_f is None else sigma_f, pb["sigma_n"])


_cache = {}


def problem(config_id, N, ds, da, H, B, shared=False, seed=None):
    """(pb, Ky_inv as numpy (ds, N, N)) of an off-grid problem, built once per process."""
    key = (config_id, N, ds, da, H, B, shared, seed)
    if key not in _cache:
        from gaussian_process_mpc_amd.synth import synth_problem
        pb = offgrid(synth_problem(config_id, N, ds, da, H, B, shared_lambda=shared), seed_of(config_id) if seed is None else seed)
        _cache[key] = (pb, bundle(pb).Ky_inv.numpy())
    return _cache[key]


def with_sigma_f(pb, sigma_f):
    """(copy of pb with other amplitudes, its Ky_inv): the SAME problem where a kernel that drops / mis-indexes the amplitude would be right."""
    q = dict(pb)
    q["sigma_f"] = np.asarray(sigma_f, dtype=np.float64).copy()
    return q, bundle(q).Ky_inv.numpy()


def assert_diag_reference_is_sane(means, vars_, cost, Q, gamma):
    """The regime where the cost is defined, re-asserted on every reference trajectory a test uses (not assumed): finite means, variances > 0,
    1 + gamma diag(Q) var > 0.  Arrays may carry leading batch dimensions."""
    means, vars_ = np.asarray(means), np.asarray(vars_)
    assert np.all(np.isfinite(means)) and np.all(np.isfinite(cost))
    assert np.all(vars_ > 0), vars_.min()
    assert np.all(1.0 + gamma * np.diag(np.asarray(Q)) * vars_ > 0)


def assert_fullcov_reference_is_sane(means, covs, cost):
    """Finite means and cost, every covariance symmetric positive definite."""
    means, covs = np.asarray(means), np.asarray(covs)
    assert np.all(np.isfinite(means)) and np.all(np.isfinite(cost))
    np.testing.assert_allclose(covs, np.swapaxes(covs, -1, -2), rtol=0, atol=1e-12 * np.abs(covs).max())
    assert np.linalg.eigvalsh(covs).min() > 0


def moved(a, b, floor=1e-300):
    """Largest relative difference of two arrays, elementwise against |b|."""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


# ------------------------------------------------------------------------------------------------------------------------------
# The shapes of tests/test_gpu_offgrid.py, shared with the discrimination check of tests/test_host_offgrid.py
# ------------------------------------------------------------------------------------------------------------------------------
LADDER_DIMS = [(1, 1), (2, 2), (3, 1), (4, 1), (5, 2), (6, 1), (7, 1)]
LADDER_N, LADDER_H = 150, 3                              # Np = 192: one 256-row tile, three 64-column chunks (tests/test_gpu_instances.py)
SHARED_DIMS = [(2, 1), (3, 1), (4, 1), (5, 1)]           # groups of 2, 3, 4 (and 2 + 2 on the split list) and 3 + 2 GPs
#                 config N     ds da H  B
WIDE_CASES = {"256x128": (21,  520,  3, 1, 3, 5),        # Np = 576: the smallest padded size beyond two 256-row tiles' 512
              "runs":    (22,  2310, 6, 1, 3, 1)}        # Np = 2368: the smallest padded size whose balanced-run list is built at ds = 6
#             tag:  (config N    ds da H   shared gamma)             the Jacobian / constraint cases of tests/test_gpu_constraints.py
JAC_CASES = {"c3": (3, 449, 4, 1, 10, False, -1.0), "d6": (4, 300, 6, 2, 8, False, -1.0)}
# action_dim >= 3 (csrc/plan.hip: no scalar-broadcast, fused or whole-horizon kernel, no step-1 quadratic form, no split: head kernel + staged
# pair_kernel.h + tail kernel at every batch): every D from 4 to 8, the three D = 8 entries with one, four and five GPs; N = LADDER_N, H = LADDER_H
WIDEACT_DIMS = [(1, 3), (2, 3), (3, 3), (2, 5), (4, 3), (1, 7), (4, 4), (5, 3)]
#               config N     ds da H          Np = 1472: the smallest padded size with more than 256 one-wave tiles per GP (23 x 24 / 2 = 276: the 64x128
WIDEACT_LONG = (472,   1415, 1, 3, 2)       # list), N no multiple of 64; 64 / (B ds) >= 2 and Np / 512 = 2: the head kernel runs in two row chunks
#                   config N    ds da shared      (H = FULLCOV_H; fullcov.hip::plan_fc2 needs da <= 2: the four-launch form at every batch, per-unit cross terms)
WIDEACT_FULLCOV = [(271,   110, 2, 3, False),
                   (272,   130, 3, 3, True),
                   (273,   110, 4, 4, False),
                   (274,   150, 5, 3, False)]
#                 config N         ds da H            nominal model, noise model, Jacobians and constraints, autograd at da >= 3; B in WIDEACT_MODEL_B
WIDEACT_MODEL = [(281,   LADDER_N, 2, 3, 4),
                 (282,   LADDER_N, 4, 4, 4)]
WIDEACT_MODEL_B = (1, 2, 5)


def ladder_config(ds, da):
    return 40 + 8 * ds + da


def shared_config(ds, da):
    return 140 + 8 * ds + da


def wideact_config(ds, da):
    # (2, 5): the seed of 200 + 8 ds + da = 221 draws a problem whose trajectory 0 -- all that the B = 1 step compares -- has a double complex cost
    # floor 60 times below that of its neighbours (1.4e-13 against 8.4e-12; tests/test_host_accuracy.py prints both): no yardstick for "10 x the
    # floor" (the staged kernel's 6.1e-13 there is what it shows on the neighbours).  521 ... 523 fail a CPU pin of their own; 524: 1.6e-12 of 1.9e-12.
    return {(2, 5): 524}.get((ds, da), 200 + 8 * ds + da)


def ladder_batches(ds):
    """Batch sizes that take a training set of one row tile through the plans (csrc/plan.hip)."""
    b_big = 5600 // ds + 3                               # ceil(B / 2) ds >= 2800 workgroups (D <= 5; B ds >= 1500 above): 256x256 tiles
    b_big += 1 - b_big % 2                               # odd: the last wave of the two-trajectory shape is half empty
    return {"one": 1, "small": 3,
            "whole_tiles": 256 // (6 * ds) + 2,          # B x 6 ds tiles of 64x64 >= 256: whole tiles per workgroup (fq = 1)
            "mid": 2048 // (3 * ds) + 2,                 # B x 3 ds >= 1700 tile workgroups: 256x64 tiles
            "big": b_big}


def shared_batches(ds):
    return {"mid": 2048 // (3 * ds) + 2, "big": max(5600 // ds + 3, 1750), "groups": 4200 // (3 * ds) + 3, "persist": 9}


def wideact_batches(ds):
    """Batch sizes of the da >= 3 plans at Np = 192.  The 256x256 list has ONE tile per GP there (wl[0][0].nwork = ds), and plan.hip takes it for
    a pack without scalar-broadcast kernels from ceil(B / 2) ds >= 1024; odd, so that the last workgroup of two trajectories carries one."""
    return {"one": 1, "small": 3, "ragged": 5, "big": 2 * (-(-1024 // ds)) + 1}


def picks(B):
    return sorted({b for b in (0, 1, B // 2, B - 1) if b < B})


def fullcov_big_batch(ds):
    units = ds + ds * (ds - 1) // 2
    return 2 * (-(-1536 // units)) + 5                   # ceil(B / 2) units >= 1536: the large-batch kernel for any padded size below 640


def gpu_rollout_shapes():
    """Every (label, problem arguments, trajectories compared, gamma, full covariance) tests/test_gpu_offgrid.py holds a rollout to the C ports on."""
    out = []
    for ds, da in LADDER_DIMS:
        bs = ladder_batches(ds)
        tr = sorted(set().union(*[picks(b) for b in list(bs.values()) + [4, 5, 6, 7]]))
        out.append(("ladder ds=%d da=%d" % (ds, da), (ladder_config(ds, da), LADDER_N, ds, da, LADDER_H, bs["big"], False), tr, -1.0, False))
    for ds, da in SHARED_DIMS:
        bs = shared_batches(ds)
        tr = sorted(set().union(*[picks(b) for b in bs.values()]))
        out.append(("shared ds=%d da=%d" % (ds, da), (shared_config(ds, da), LADDER_N, ds, da, LADDER_H, max(bs.values()), True), tr, -1.0, False))
    for tag, (cfg, N, ds, da, H, B) in WIDE_CASES.items():
        out.append((tag, (cfg, N, ds, da, H, B, False), picks(B), -1.0, False))
    for cfg, N, ds, da, shared in FULLCOV_CASES:
        B = fullcov_big_batch(ds)
        out.append(("fullcov ds=%d da=%d" % (ds, da), (cfg, N, ds, da, FULLCOV_H, B, shared), sorted(set().union(*[picks(b) for b in (1, 2, 3, 5, B)])), -1.0, True))
    for ds, da in WIDEACT_DIMS:
        bs = wideact_batches(ds)
        tr = sorted(set().union(*[picks(b) for b in bs.values()]))
        out.append(("wideact ds=%d da=%d" % (ds, da), (wideact_config(ds, da), LADDER_N, ds, da, LADDER_H, bs["big"], False), tr, -1.0, False))
    cfg, N, ds, da, H = WIDEACT_LONG
    out.append(("wideact long N=%d" % N, (cfg, N, ds, da, H, 2, False), [0, 1], -1.0, False))
    for cfg, N, ds, da, shared in WIDEACT_FULLCOV:
        B = fullcov_big_batch(ds)
        out.append(("wideact fullcov ds=%d da=%d" % (ds, da), (cfg, N, ds, da, FULLCOV_H, B, shared), sorted(set().union(*[picks(b) for b in (1, 2, 3, 5, B)])), -1.0, True))
    for cfg, N, ds, da, H in WIDEACT_MODEL:
        out.append(("wideact model ds=%d da=%d" % (ds, da), (cfg, N, ds, da, H, max(WIDEACT_MODEL_B), False), list(range(max(WIDEACT_MODEL_B))), -1.0, False))
    for cfg, N, ds, da, H, shared, gamma in (DIAG_CASES[0], DIAG_CASES[2], DIAG_CASES[3]):      # nominal packs, life cycle and class path
        out.append(("case %d N=%d%s" % (cfg, N, " shared" if shared else ""), (cfg, N, ds, da, H, 64, shared), [0, 1, 2, 63], gamma, False))
    for tag, (cfg, N, ds, da, H, shared, gamma) in JAC_CASES.items():
        out.append(("jacobian " + tag, (cfg, N, ds, da, H, 2, shared), [0, 1], gamma, False))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# The step tables of tests/test_gpu_offgrid.py (parity with the C ports at the project tolerances) and tests/test_gpu_accuracy.py (the
# rounding-error budget): which batch, under which GPMPC_* overrides, reaches which kernel form.  Both modules iterate these.
# ------------------------------------------------------------------------------------------------------------------------------
NO_PERSIST = {"GPMPC_PERSIST": "0"}        # (a small training set in a large batch is planned as the whole-horizon kernel: the step-per-launch forms are asked for)
LADDER_EXPECTED = {("fused_staged", "64x64", "quarter columns"), ("fused_staged", "64x64", "whole tiles"), ("head+pair_sb", "256x64", "tb1"),
                   ("fused_sb", "256x64", ""), ("fused_sb", "256x32", ""), ("fused_sb", "256x16", ""), ("persist", "", "16 waves"),
                   ("persist", "", "8 waves"), ("head+pair_sb", "256x256", "big"), ("head+pair_staged", "64x64", "")}


def ladder_steps(ds):
    """The diagonal form ladder at N = LADDER_N: (B, overrides, form, tiling, tag, how the kernel name shows it)."""
    bs = ladder_batches(ds)
    narrow = {"GPMPC_FUSED_SB": "1", "GPMPC_PAIR_SB": "1"}
    return [(bs["small"],       {},                                         "fused_staged",     "64x64",   "quarter columns", ",4,1>"),
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


def assert_ladder_plan(plan, step, D):
    """The plan of a ladder step is the form the step is meant for."""
    B, env, form, tiling, tag, kern = step
    assert plan["form"] == form and (not tiling or plan["tiling"] == tiling) and kern in plan["kernel"], (B, env, plan)
    if tag == "big":                              # two trajectories per wave up to D = 5: the odd batch leaves the last wave half empty
        assert plan["tb"] == (2 if D <= 5 else 1) and B % 2 == 1, plan
    if tag == "tb1":
        assert plan["tb"] == 1, plan


WIDEACT_EXPECTED = {("head+pair_staged", "64x64", 1, "eager"), ("head+pair_staged", "64x64", 2, "eager"), ("head+pair_staged", "64x64", 2, "graph"),
                    ("head+pair_staged", "64x64", 4, "eager"), ("head+pair_staged", "256x256", 2, "eager"), ("head+pair_staged", "256x256", 1, "eager")}
WIDEACT_LONG_EXPECTED = {("head+pair_staged", "64x128", 1, "eager"), ("head+pair_staged", "64x128", 2, "eager")}
# overrides that select among kernels a da >= 3 pack does not have: the plan and every bit of the result stay what they were
WIDEACT_INERT = [{"GPMPC_PERSIST": "16"}, {"GPMPC_FUSED_SB": "1"}, {"GPMPC_PAIR_SB": "1"}, {"GPMPC_TILING": "2"}, {"GPMPC_TILING": "5"}, {"GPMPC_STEP1_QUAD": "1"}]
WIDEACT_INERT_DIMS = [(2, 3), (4, 4)]                     # one of D = 5, one of D = 8


def wideact_steps(ds):
    """The da >= 3 plans at N = LADDER_N: (B, overrides, form, tiling, trajectories per workgroup, "eager" | "graph")."""
    bs = wideact_batches(ds)
    st = "head+pair_staged"
    return [(bs["one"],    {},                     st, "64x64",   1, "eager"),
            (bs["small"],  {},                     st, "64x64",   2, "eager"),       # odd: the last workgroup carries one trajectory
            (bs["small"],  {},                     st, "64x64",   2, "graph"),       # the same plan, replayed as a captured graph
            (bs["ragged"], {"GPMPC_PAIR_TB": "4"}, st, "64x64",   4, "eager"),       # 4 + 1 trajectories
            (bs["big"],    {},                     st, "256x256", 2, "eager"),
            (bs["big"],    {"GPMPC_PAIR_TB": "1"}, st, "256x256", 1, "eager")]


def wideact_long_steps():
    st = "head+pair_staged"
    return [(1, {}, st, "64x128", 1, "eager"), (2, {}, st, "64x128", 2, "eager")]


WIDEACT_CASES = [(ds, da, LADDER_N) for ds, da in WIDEACT_DIMS] + [WIDEACT_LONG[2:4] + (WIDEACT_LONG[1],)]      # (ds, da, N): the ladder and its long case


def wideact_case(ds, da, N):
    """(problem arguments, steps, expected set) of a WIDEACT_CASES entry."""
    if N == LADDER_N:
        return (wideact_config(ds, da), N, ds, da, LADDER_H, wideact_batches(ds)["big"], False), wideact_steps(ds), WIDEACT_EXPECTED
    cfg, N, ds, da, H = WIDEACT_LONG
    return (cfg, N, ds, da, H, 2, False), wideact_long_steps(), WIDEACT_LONG_EXPECTED


def assert_wideact_plan(plan, step, D):
    """The plan of a da >= 3 step: head kernel + the fp64 staged pair kernel + tail kernel, unsplit, no step-1 quadratic form."""
    B, env, form, tiling, tb, mode = step
    assert plan["form"] == form and plan["tiling"] == tiling and plan["tb"] == tb, (B, env, plan)
    assert "gpmpc_pair_kernel<%d,true," % D in plan["kernel"] and plan["kernel"].endswith(",%d>" % tb), (B, env, plan)
    assert plan["launches_per_step"] == 2 and plan["split"] == 1 and plan["shared"] == 0 and "step1" not in plan, (B, env, plan)
    if tiling == "64x128":
        assert plan["hchunks"] >= 2, plan                 # the head kernel's row chunks feed the staged kernel
    else:
        assert tb == 1 or B % tb != 0, (B, tb)            # more than one trajectory per workgroup: the last workgroup is ragged


def wide_step(tag):
    """(overrides, assertion on the plan) of a WIDE_CASES entry."""
    if tag == "256x128":
        def check(plan):
            assert plan["form"] == "head+pair_sb" and plan["tiling"] == "256x128" and plan["tb"] == 2, plan
        return {"GPMPC_PAIR_SB": "1", "GPMPC_TILING": "4"}, check

    def check(plan):
        assert plan["form"] == "fused_sb" and plan["tiling"] == "256x256" and ",256,1>" in plan["kernel"] and plan["launches_per_step"] == 1, plan
    return {}, check


def shared_steps(ds):
    """The one-lambda forms at N = LADDER_N, da = 1: (B, overrides, form, tiling, how the kernel name shows it)."""
    bs = shared_batches(ds)
    group = {2: 2, 3: 3, 4: 4, 5: 3}[ds]                      # gpmpc_sbs_group at da = 1
    all_in_one = ds in (3, 4)
    fsb = {"GPMPC_FUSED_SB": "1"}
    steps = [(bs["mid"],     NO_PERSIST,               "head+pair_sbs",   "256x64",  ",%d,%d," % (group, ds)),
             (bs["big"],     NO_PERSIST,               "head+pair_sbs",   "256x256", ",%d,%d," % (group, ds)),
             (bs["mid"],     fsb,                      "fused_sb_shared", "256x64",  ",0,%d>" % (2 if ds == 4 else group)),      # ds = 4: the 2 + 2 split list
             (bs["persist"], {"GPMPC_PERSIST": "16"},  "persist",         "",        ",%d>x16waves" % (ds if all_in_one else 2)),
             (bs["persist"], {"GPMPC_PERSIST": "8"},   "persist",         "",        ",2>x8waves")]
    if ds == 4:
        steps.insert(3, (bs["groups"], fsb,            "fused_sb_shared", "256x64",  ",0,4>"))                                   # >= 4200 tile workgroups: all four GPs
    return steps


def assert_shared_plan(plan, step):
    B, env, form, tiling, kern = step
    assert plan["form"] == form and (not tiling or plan["tiling"] == tiling) and kern in plan["kernel"].replace(" ", ""), (B, env, plan)


def fullcov_steps(ds, shared):
    """The full-covariance forms: (B, overrides, form).  The two-launch form on each of its tilings, the four-launch form at a small and a
    large batch; with one lambda, the cross-unit kernel forced on (ds <= 4; its per-unit fallback at ds = 5)."""
    b_big = fullcov_big_batch(ds)
    two = {"GPMPC_FC_FORM": "1"}
    cases = [(3, {}, "two_launch"), (b_big, {}, "two_launch"), (3, dict(two, GPMPC_FC_TILING="4"), "two_launch"), (2, dict(two, GPMPC_FC_TILING="0"), "two_launch"),
             (1, dict(two, GPMPC_FC_TILING="2"), "two_launch"), (3, {"GPMPC_FC_FORM": "0"}, "four_launch"), (b_big, {"GPMPC_FC_FORM": "0"}, "four_launch")]
    if shared:
        forced = {"GPMPC_FC_SHARED": "1"}
        cases += [(1, forced, "two_launch"), (3, forced, "two_launch"), (5, dict(forced, GPMPC_FC_TILING="4"), "two_launch"),
                  (2, dict(forced, GPMPC_FC_TILING="0"), "two_launch")]
    return cases


def assert_fullcov_plan(plan, step, ds, da=1):
    """The plan of a full-covariance step; returns a word on the cross units for the label.  da >= 3: fullcov.hip::plan_fc2 has no instance, so every
    step of ``fullcov_steps`` -- whatever it asks for -- is the four-launch form with per-unit cross terms (GPMPC_FC_FORM, _TILING, _SHARED inert)."""
    B, env, form = step
    if da > 2:
        assert plan["form"] == "four_launch" and plan["shared_cross_units"] == 0, (env, plan)
        return " four-launch, cross units per unit"
    assert plan["form"] == form, (env, plan)
    if "GPMPC_FC_SHARED" in env:
        assert plan["shared_cross_units"] == (1 if ds <= 4 else 0), plan
        return " cross units %s" % ("pair_kernel_sbfx.h" if plan["shared_cross_units"] else "per unit")
    if form == "two_launch" and B <= 5:
        assert plan["shared_cross_units"] == 0, plan           # (the shared cross-unit kernel is planned from B Np^2 pairs >= 3.5e7)
    return ""
