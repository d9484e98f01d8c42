"""The yardstick of tests/test_gpu_accuracy.py, checked without a GPU: oracle/cport/gpmpc_cpu_given.c (one step and the whole rollout on given
constants, in double and long double, real and complex) is pinned to the existing ports; K_ref -- the rounding error of the plain fp64
evaluation of the reference formula in units of 2^-53 x (sum of the absolute terms) -- is recorded for every problem the GPU test uses; and the
budget is shown to DISCRIMINATE: emulated defects that pass the project tolerances (OG.GPU_*_RTOL) miss the budget (OG.BUDGET_K).

K_ref measured here (worst over the compared trajectories and steps; means | variances | covariances):
    ladder (N = 150, H = 3)  ds = 1: 0.80 | 0.13    2: 0.79 | 0.38    3: 0.91 | 0.26    4: 1.7 | 0.37    5: 0.69 | 0.28    6: 0.84 | 0.40    7: 1.4 | 0.57
    one lambda (N = 150)     ds = 2: 0.52 | 0.50    3: 0.93 | 0.27    4: 0.75 | 0.25    5: 1.1 | 0.37
    256x128 (N = 520): 0.85 | 0.44        balanced runs (N = 2310): 0.92 | 0.32
    full covariance          ds = 2: 1.0 | 0.29 | 0.29    3: 0.61 | 0.36 | 0.36    4: 1.3 | 0.33 | 0.33    5: 1.2 | 0.34 | 0.34    6: 1.0 | 0.22 | 0.22
    action_dim >= 3 (N = 150, H = 3)  (1, 3): 0.27 | 0.19    (2, 3): 0.47 | 0.24    (3, 3): 1.4 | 0.31    (2, 5): 0.53 | 0.20    (4, 3): 1.0 | 0.15
                             (1, 7): 0.48 | 0.24    (4, 4): 1.8 | 0.37    (5, 3): 1.2 | 0.31    long case (N = 1415): 0.16 | 0.29
    full covariance, da >= 3 (2, 3): 0.98 | 0.24 | 0.24    (3, 3): 0.65 | 0.23 | 0.23    (4, 4): 1.1 | 0.19 | 0.20    (5, 3): 0.94 | 0.20 | 0.24
    (all within OG.BUDGET_K; their double complex floors: cost 8.8e-10 and gradient 1.2e-9 at most, the largest at N = 1415 and at (1, 3):
    test_wide_action_yardstick_is_within_the_budget)
The variances sit at 0.13 ... 0.57 (not the 0.03 ... 0.05 of a single step: these are maxima over 3 ... 39 steps and all GPs, and the compiler
contracts multiply-adds; another build of the same source moved single entries by a factor 2), with sum|terms| / var from 3.5e4 (ds = 7) to 1.1e11
(N = 2310): the unit holds over six orders of magnitude of conditioning.  Weighted with the expanded exponent of the HIP kernels
(q_i + q_j + 2 sum |h_ik h_jk| per term) the absolute sum is 0.5 ... 2.5 A_var.

Defects emulated in the double result of one step (teacher forcing: the inputs of step 2 of trajectory 0), each as a multiple of the project
tolerance | of the budget:
    one table step     ds = 1, 2: the glitch of EVERY pair already misses the tolerance (the variance is 1e-9 of its terms): no gap (NO_GAP).
                       ds = 3: one pair of one GP passes (0.47 | 642).  ds = 4: 9 ... 472 of 11325 pairs pass, the largest at 1 | 4e4 ... 1e6.
                       ds = 5, 6: 240 ... 5400 pairs pass, ds = 7: 9500 ... 11200; the largest at 1 | 3e6 ... 2.5e9.  The budget sees every pair
                       at every dimension.
    quarter of a chunk misses the tolerance everywhere (45 ... 5e9 tolerances; 3e10 ... 7e12 budgets).  The largest lowest-|weight| subset that
                       passes: none at ds <= 3 (NO_GAP); at ds = 4 ... 7, where a GP has one, 0.5 ... 1 | 1e6 ... 2e9.
    action variance    passes both tolerances by 1e-3 ... 1e-8.  Variance K: 0.11, 0.38, 0.09, 0.54 (ds = 1 ... 4: inside the budget of 0.7), 15, 18,
                       460 (ds = 5 ... 7).  Mean K: 7.0, 13, 13, 160, 2e3, 1e3, 6e3 against the budget of 2: separated at every dimension.
    swapped weights    (full covariance) 1.9e3 ... 3.5e7 tolerances: the project tolerance catches it on every unit; 7e8 ... 5e12 budgets.
    cross unit, one table step   ds = 2: no pair passes the tolerance (NO_GAP); ds = 4: 1 | 850; ds = 6: 1 | 4e6 ... 4e7.
"""
import numpy as np
import pytest

import offgrid_problems as OG

U53 = 2.0 ** -53
ACT_VAR = float(np.float32(1e-3))
THREADS = 8

# cport vs cport: two fp64 evaluations of the same sums on constants rounded differently -- the tolerances tests/test_host_offgrid.py pins the
# existing ports to the torch oracle with (its header: measured deviation x 10, never above a tenth of the GPU tolerance)
DIAG_MEAN_RTOL, DIAG_MEAN_ATOL, DIAG_VAR_RTOL, DIAG_COST_RTOL, DIAG_GRAD_RTOL, DIAG_GRAD_ATOL = 3e-7, 1e-10, 1e-6, 1e-8, 1e-6, 1e-9
FC_MEAN_RTOL, FC_MEAN_ATOL, FC_COV_RTOL, FC_COV_ATOL_OF_MAX, FC_COST_RTOL, FC_DDIR_RTOL, FC_DDIR_ATOL = 1e-9, 1e-11, 1e-6, 8e-8, 1e-9, 1e-7, 1e-10

# K_ref of a plain fp64 evaluation, first order: every term carries the rounding of its exponent (|argument| 2^-53; the arguments of the terms
# that matter are of order 1 ... 10) and of one multiply-add, with random signs over the terms of the sum.  The N^2 / 2 terms of a variance
# average that below one unit; the N terms of a mean (and their larger arguments, -q / 2 with q the full quadratic form) do not.  A plain
# evaluation beyond these would be a systematic error of the yardstick itself.
K_REF_MAX = {"mean": 4.0, "var": 1.0, "cov": 1.0}

SHAPES = [s for s in OG.gpu_rollout_shapes() if s[0].split(" ")[0] in ("ladder", "shared", "256x128", "runs", "fullcov")
          or s[0].startswith(("wideact ds", "wideact long", "wideact fullcov"))]
_IDS = [s[0].replace(" ", "-") for s in SHAPES]


def _K(got, ld, A):
    return float(np.max(np.abs(got - ld) / (U53 * A)))


def _inputs_diag(pb, tr, means, vars_):
    H, ds, da = pb["H"], pb["ds"], pb["da"]
    u = np.concatenate([means[:, :H], pb["U"][tr]], axis=2).reshape(-1, ds + da)
    s = np.concatenate([vars_[:, :H], np.full((len(tr), H, da), ACT_VAR)], axis=2).reshape(-1, ds + da)
    return u, s


def _inputs_full(pb, tr, means, covs):
    H, ds, da = pb["H"], pb["ds"], pb["da"]
    D = ds + da
    u = np.concatenate([means[:, :H], pb["U"][tr]], axis=2).reshape(-1, D)
    S = np.zeros((len(tr), H, D, D))
    S[:, :, :ds, :ds] = covs[:, :H]
    S[:, :, np.arange(ds, D), np.arange(ds, D)] = ACT_VAR
    return u, S.reshape(-1, D, D)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the new code is pinned
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds,da", OG.LADDER_DIMS)
def test_long_double_trajectory_equals_the_x87_rollout(ds, da):
    """The long double build on constants computed in long double from Ky_inv performs the operations of gpmpc_cpu_rollout_ld in the same
    order: the two agree to the last rounding, which is the conversion of the result to fp64 (one ulp allowed; measured: bit for bit)."""
    from oracle import cport
    pb, kinv = OG.problem(OG.ladder_config(ds, da), OG.LADDER_N, ds, da, OG.LADDER_H, 3, False)
    beta, W = cport.constants_ld(pb, kinv)
    g = cport.given_rollout(pb, beta, W, -1.0, prec="ld", nthreads=THREADS)
    e = cport.rollout_extended(pb, kinv, nthreads=THREADS)
    print("ld trajectory vs gpmpc_cpu_rollout_ld: means %.2e variances %.2e" % (OG.moved(g["means"], e["means"]), OG.moved(g["vars"], e["vars"])))
    assert np.all(np.abs(g["means"] - e["means"]) <= 2.0 ** -52 * np.abs(e["means"]))
    assert np.all(np.abs(g["vars"] - e["vars"]) <= 2.0 ** -52 * np.abs(e["vars"]))


@pytest.mark.parametrize("gamma", [-1.0, 1e-5, 0.0])
@pytest.mark.parametrize("ds,da", [(1, 1), (3, 1), (5, 2), (7, 1)])
def test_double_builds_agree_with_the_diagonal_port(ds, da, gamma):
    """double build vs cport.rollout (means, variances, cost: general Q, x_ref, u_ref, gamma < 0, > 0 and = 0) and the complex-step gradient of
    the double complex build vs its analytic adjoint, on the numpy-definition constants."""
    from oracle import cport
    pb, kinv = OG.problem(OG.ladder_config(ds, da), OG.LADDER_N, ds, da, OG.LADDER_H, 3, False)
    beta, W = cport.constants(pb, kinv)
    c = cport.rollout(pb, kinv, gamma, nthreads=THREADS)
    OG.assert_diag_reference_is_sane(c["means"], c["vars"], c["cost"], pb["Q"], gamma)
    d = cport.given_rollout(pb, beta, W, gamma, prec="d", nthreads=THREADS)
    g = cport.given_rollout(pb, beta, W, gamma, prec="cd", nthreads=THREADS)
    gerr = np.linalg.norm(g["grad"] - c["grad"]) / np.linalg.norm(c["grad"])
    print("ds=%d gamma=%g: means %.2e vars %.2e cost %.2e | complex step: cost %.2e grad (norm) %.2e" % (
        ds, gamma, OG.moved(d["means"], c["means"], 1e-10), OG.moved(d["vars"], c["vars"]), OG.moved(d["cost"], c["cost"]), OG.moved(g["cost"], c["cost"]), gerr))
    np.testing.assert_allclose(d["means"], c["means"], rtol=DIAG_MEAN_RTOL, atol=DIAG_MEAN_ATOL)
    np.testing.assert_allclose(d["vars"], c["vars"], rtol=DIAG_VAR_RTOL)
    np.testing.assert_allclose(d["cost"], c["cost"], rtol=DIAG_COST_RTOL)
    np.testing.assert_allclose(g["cost"], c["cost"], rtol=DIAG_COST_RTOL)
    np.testing.assert_allclose(g["grad"], c["grad"], rtol=DIAG_GRAD_RTOL, atol=DIAG_GRAD_ATOL)
    assert gerr <= DIAG_GRAD_RTOL


@pytest.mark.parametrize("case", OG.FULLCOV_CASES, ids=lambda c: "ds%d-da%d-N%d%s" % (c[2], c[3], c[1], "-shared" if c[4] else ""))
def test_double_builds_agree_with_the_full_covariance_port(case):
    """double build vs cport.rollout_fullcov (means, covariances, cost) and the complex-step gradient of the double complex build along two seeded
    directions vs the port's own complex step."""
    from oracle import cport
    cfg, N, ds, da, shared = case
    H, B = OG.FULLCOV_H, OG.FULLCOV_B
    pb, kinv = OG.problem(cfg, N, ds, da, H, B, shared)
    beta, W = cport.constants(pb, kinv)
    dirs = np.random.default_rng(cfg).normal(size=(B, 2, H, da))
    c = cport.rollout_fullcov(pb, kinv, -1.0, dirs=dirs, nthreads=THREADS)
    OG.assert_fullcov_reference_is_sane(c["means"], c["covs"], c["cost"])
    d = cport.given_rollout(pb, beta, W, -1.0, full=True, prec="d", nthreads=THREADS)
    g = cport.given_rollout(pb, beta, W, -1.0, full=True, prec="cd", nthreads=THREADS)
    dd = np.einsum("bhk,bdhk->bd", g["grad"], dirs)
    scale = np.abs(c["covs"]).max()
    print("fullcov ds=%d: means %.2e covs %.2e of the largest cost %.2e ddir %.2e" % (
        ds, OG.moved(d["means"], c["means"], 1e-11), np.abs(d["covs"] - c["covs"]).max() / scale, OG.moved(d["cost"], c["cost"]), OG.moved(dd, c["ddir"], 1e-10)))
    np.testing.assert_allclose(d["means"], c["means"], rtol=FC_MEAN_RTOL, atol=FC_MEAN_ATOL)
    np.testing.assert_allclose(d["covs"], c["covs"], rtol=FC_COV_RTOL, atol=FC_COV_ATOL_OF_MAX * scale)
    np.testing.assert_allclose(d["cost"], c["cost"], rtol=FC_COST_RTOL)
    np.testing.assert_allclose(g["cost"], c["cost"], rtol=FC_COST_RTOL)
    np.testing.assert_allclose(dd, c["ddir"], rtol=FC_DDIR_RTOL, atol=FC_DDIR_ATOL)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. K_ref on every problem of the GPU test
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_k_ref_of_the_plain_fp64_evaluation(shape):
    """Per step, on the trajectories the GPU test compares: the double build against the long double build on the same numpy-definition
    constants and the same inputs (the double trajectory's own outputs of the step before)."""
    from oracle import cport
    label, args, tr, gamma, full = shape
    pb, kinv = OG.problem(*args)
    ds = pb["ds"]
    beta, W = cport.constants(pb, kinv)
    t = cport.given_rollout(pb, beta, W, gamma, x0=pb["x0"][tr], U=pb["U"][tr], full=full, prec="d", nthreads=THREADS)
    if full:
        u, S = _inputs_full(pb, tr, t["means"], t["covs"])
        d = cport.given_step_full(pb, beta, W, u, S, prec="d", nthreads=THREADS)
        ld = cport.given_step_full(pb, beta, W, u, S, prec="ld", nthreads=THREADS)
        assert np.array_equal(d["cov"], t["covs"][:, 1:].reshape(-1, ds, ds))                # the step entry is the trajectory's step
        assert np.linalg.eigvalsh(ld["cov"]).min() > 0
        dg = np.arange(ds)
        k = {"mean": _K(d["mean"], ld["mean"], ld["A_mean"]), "var": _K(d["cov"][:, dg, dg], ld["cov"][:, dg, dg], ld["A_cov"][:, dg, dg]),
             "cov": _K(d["cov"], ld["cov"], ld["A_cov"])}
        ratio = float((ld["A_cov"][:, dg, dg] / ld["cov"][:, dg, dg]).max())
    else:
        u, s = _inputs_diag(pb, tr, t["means"], t["vars"])
        d = cport.given_step_diag(pb, beta, W, u, s, prec="d", nthreads=THREADS)
        ld = cport.given_step_diag(pb, beta, W, u, s, prec="ld", nthreads=THREADS)
        assert np.array_equal(d["var"], t["vars"][:, 1:].reshape(-1, ds)) and np.array_equal(d["mean"], t["means"][:, 1:].reshape(-1, ds))
        assert np.all(ld["var"] > 0)
        k = {"mean": _K(d["mean"], ld["mean"], ld["A_mean"]), "var": _K(d["var"], ld["var"], ld["A_var"])}
        ratio = float((ld["A_var"] / ld["var"]).max())
    print("K_REF %s (%d trajectories x %d steps): %s; cancellation sum|terms| / var up to %.3g%s" % (
        label, len(tr), pb["H"], " ".join("%s %.3g" % kv for kv in k.items()), ratio,
        "" if full else "; expanded exponent: A_exp / A_var up to %.3g" % float((ld["A_exp"] / ld["A_var"]).max())))
    for q, v in k.items():
        assert v <= K_REF_MAX[q], (label, q, v)


_WIDEACT = [s for s in SHAPES if s[0].startswith("wideact")]


@pytest.mark.parametrize("shape", _WIDEACT, ids=[s[0].replace(" ", "-") for s in _WIDEACT])
def test_wide_action_yardstick_is_within_the_budget(shape):
    """The action_dim >= 3 problems of tests/test_gpu_accuracy.py, on the trajectories it compares: K_ref of the double build lies within
    OG.BUDGET_K, and the floors -- cost and gradient (in norm) of the double complex build against the long double complex step -- within
    OG.BUDGET_TRAJ, so that on these problems the budget can only be exceeded by the kernels.  Printed as well: the floor of trajectory 0 alone,
    the whole yardstick of the B = 1 steps (a double evaluation that happens to land 60 times closer than its neighbours -- seed 221 at ds = 2,
    da = 5 -- measures nothing; OG.wideact_config).  (A drawn problem that fails this gets another config id, not another budget.)"""
    from oracle import cport
    label, args, tr, gamma, full = shape
    pb, kinv = OG.problem(*args)
    ds = pb["ds"]
    beta, W = cport.constants(pb, kinv)
    kw = dict(x0=pb["x0"][tr], U=pb["U"][tr], full=full, nthreads=THREADS)
    t = cport.given_rollout(pb, beta, W, gamma, prec="d", **kw)
    if full:
        OG.assert_fullcov_reference_is_sane(t["means"], t["covs"], t["cost"])
        u, S = _inputs_full(pb, tr, t["means"], t["covs"])
        d = cport.given_step_full(pb, beta, W, u, S, prec="d", nthreads=THREADS)
        ld = cport.given_step_full(pb, beta, W, u, S, prec="ld", nthreads=THREADS)
        dg = np.arange(ds)
        k = {"mean": _K(d["mean"], ld["mean"], ld["A_mean"]), "var": _K(d["cov"][:, dg, dg], ld["cov"][:, dg, dg], ld["A_cov"][:, dg, dg]),
             "cov": _K(d["cov"], ld["cov"], ld["A_cov"])}
    else:
        OG.assert_diag_reference_is_sane(t["means"], t["vars"], t["cost"], pb["Q"], gamma)
        u, s = _inputs_diag(pb, tr, t["means"], t["vars"])
        d = cport.given_step_diag(pb, beta, W, u, s, prec="d", nthreads=THREADS)
        ld = cport.given_step_diag(pb, beta, W, u, s, prec="ld", nthreads=THREADS)
        k = {"mean": _K(d["mean"], ld["mean"], ld["A_mean"]), "var": _K(d["var"], ld["var"], ld["A_var"])}
    cld = cport.given_rollout(pb, beta, W, gamma, prec="cld", **kw)
    cd = cport.given_rollout(pb, beta, W, gamma, prec="cd", **kw)
    each = {"cost": np.abs(cd["cost"] - cld["cost"]) / np.abs(cld["cost"]),
            "grad": np.array([np.linalg.norm(cd["grad"][b] - cld["grad"][b]) / np.linalg.norm(cld["grad"][b]) for b in range(len(tr))])}
    floor = {q: float(v.max()) for q, v in each.items()}
    print("YARDSTICK %s: K_ref %s; floors cost %.3g grad %.3g, of trajectory 0 alone %.3g %.3g" % (
        label, " ".join("%s %.3g" % kv for kv in k.items()), floor["cost"], floor["grad"], each["cost"][0], each["grad"][0]))
    assert tr[0] == 0
    for q, v in k.items():
        assert v <= OG.BUDGET_K[q], (label, q, v)
    for q, v in floor.items():
        assert v <= OG.BUDGET_TRAJ[q], (label, q, v)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the budget discriminates
# ------------------------------------------------------------------------------------------------------------------------------
TABLE_STEP = 2.0 ** (1.0 / 2048.0) - 1.0                # one step of the exp table (csrc/fast_exp.h): 3.4e-4 of the term
# (defect, dimension) the per-step budget cannot separate, with the reason; everything else is asserted.  Empty: the action variance, the one
# candidate (at ds <= 4 sum|terms| / var is 1e7 and more, and 2^-53 A_var exceeds the effect of its 4.7e-8 relative change on the VARIANCE), is
# separated at every dimension by the budget on the MEAN, whose sum does not cancel.
NOT_SEPARATED = {}
# (defect, dimension) where no instance of the defect passes the project tolerance in the first place: the variance is so small against its
# terms (1e-9 of them) that the smallest affected term already moves it by more than 1e-4.  There is no gap to show there; the budget sees them too.
NO_GAP = {("one table step", 1), ("one table step", 2), ("cross unit, one table step", 2), ("quarter of a chunk", 1), ("quarter of a chunk", 2),
          ("quarter of a chunk", 3)}


def _pair_terms(pb, W, a, u, s):
    """The N x N terms W_ij E_ij of GP a's variance sum at the input N(u, diag(s)), [j][i] as the weights are stored, and the factor c."""
    X, lam = pb["X"], pb["lambdas"][a]
    N = X.shape[0]
    h = np.sqrt(0.125 / (0.5 * lam + s)) * (u - X)
    T = W[a][:N, :N] * np.exp(-((h[:, None, :] + h[None, :, :]) ** 2).sum(axis=2))
    return 1.0 / np.sqrt(np.prod(2.0 * s / lam + 1.0)), T


def _step2_inputs(pb, beta, W, full):
    """The inputs of step 2 of trajectory 0 (the double trajectory's own step 1)."""
    from oracle import cport
    ds, da = pb["ds"], pb["da"]
    t = cport.given_rollout(pb, beta, W, -1.0, x0=pb["x0"][:1], U=pb["U"][:1], full=full, prec="d", nthreads=THREADS)
    u = np.concatenate([t["means"][0, 1], pb["U"][0, 1]])
    if not full:
        return u, np.concatenate([t["vars"][0, 1], np.full(da, ACT_VAR)])
    S = np.zeros((ds + da, ds + da))
    S[:ds, :ds] = t["covs"][0, 1]
    S[np.arange(ds, ds + da), np.arange(ds, ds + da)] = ACT_VAR
    return u, S


def _largest_that_passes(d, old):
    """Of the deviations d, the largest the project tolerance passes (None: it passes none)."""
    ok = old(d) <= 1.0
    return float(np.abs(d[ok]).max()) if ok.any() else None


@pytest.mark.parametrize("ds,da", OG.LADDER_DIMS)
def test_budget_separates_defects_the_project_tolerances_pass(ds, da):
    """Defects emulated in the double result of one diagonal step, per GP; each in units of the project tolerance on the variance
    (|d| / (1e-4 var + 1e-12), passes at <= 1) and of the budget (|d| / (2^-53 A_var), fails above OG.BUDGET_K).

    one table step      ONE pair's term scaled by 2^(1/2048).  The variance cancels to 1e-4 ... 1e-9 of its terms, so a glitch in one of the LARGE
                        pairs already misses the project tolerance; the pairs it cannot see are the gap.  Taken: the largest pair whose glitch
                        still passes the tolerance.  Printed: how many of the pairs either check sees.
    quarter of a chunk  the lowest-|weight| quarter of the pairs in the last (ragged) 64-column chunk dropped.  That misses the project
                        tolerance at every dimension here (printed) and the budget by far more; the gap is shown on the largest
                        lowest-|weight| subset of the chunk that the tolerance still passes.
    action variance     1e-3 instead of float32(1e-3): variance and mean of every GP; separated when one of them misses its budget.  The variance
                        alone separates it at ds >= 5 only (printed); the mean at every dimension.
    NO_GAP lists the dimensions at which the tolerance passes no instance of a defect; the list is asserted to be exact."""
    from oracle import cport
    pb, kinv = OG.problem(OG.ladder_config(ds, da), OG.LADDER_N, ds, da, OG.LADDER_H, 3, False)
    N = pb["X"].shape[0]
    beta, W = cport.constants(pb, kinv)
    u, s = _step2_inputs(pb, beta, W, False)
    d = cport.given_step_diag(pb, beta, W, u, s, prec="d", nthreads=THREADS)
    ld = cport.given_step_diag(pb, beta, W, u, s, prec="ld", nthreads=THREADS)
    s_wrong = s.copy()
    s_wrong[ds:] = 1e-3
    w = cport.given_step_diag(pb, beta, W, u, s_wrong, prec="d", nthreads=THREADS)
    bad, act, gap = [], 0.0, {"one table step": False, "quarter of a chunk": False}
    jj, ii = np.tril_indices(N)
    chunk = jj >= 64 * ((N - 1) // 64)                                           # the pairs (i <= j) of the last column chunk
    for a in range(ds):
        var, A = d["var"][0, a], ld["A_var"][0, a]
        c, T = _pair_terms(pb, W, a, u, s)
        assert abs(pb["sigma_f"][a] ** 2 - c * T.sum() - d["mean"][0, a] ** 2 - var) <= 2.0 * U53 * A           # these ARE the terms of the C step
        old = lambda dv: np.abs(dv) / (OG.GPU_VAR_RTOL * abs(var) + 1e-12)      # noqa: E731
        new = lambda dv: np.abs(dv) / (U53 * A)                                 # noqa: E731
        g = c * np.abs(T[jj, ii]) * TABLE_STEP
        assert new(g.min()) > OG.BUDGET_K["var"] or old(g.min()) <= 1.0
        pick = _largest_that_passes(g, old)
        print("DEFECT ds=%d GP %d one table step: of %d pairs the tolerance sees %d, the budget %d; the largest pair the tolerance passes: %s" % (
            ds, a, g.size, (old(g) > 1.0).sum(), (new(g) > OG.BUDGET_K["var"]).sum(), "none" if pick is None else "%.3g | %.3g" % (old(pick), new(pick))))
        if pick is not None:
            gap["one table step"] = True
            if not new(pick) > OG.BUDGET_K["var"]:
                bad.append(("one table step", a, new(pick)))
        order = np.argsort(np.abs(W[a][jj[chunk], ii[chunk]]), kind="stable")
        drops = c * np.cumsum(T[jj[chunk], ii[chunk]][order])                    # the k lowest-|weight| pairs of the chunk dropped, k = 1 ...
        q = drops[chunk.sum() // 4 - 1]
        pick = _largest_that_passes(drops, old)
        print("DEFECT ds=%d GP %d quarter of a chunk (%d of %d pairs): %.3g | %.3g; the largest lowest-|weight| subset the tolerance passes: %s" % (
            ds, a, chunk.sum() // 4, chunk.sum(), old(q), new(q), "none" if pick is None else "%.3g | %.3g" % (old(pick), new(pick))))
        if not new(q) > OG.BUDGET_K["var"]:
            bad.append(("quarter of a chunk, whole", a, new(q)))
        if pick is not None:
            gap["quarter of a chunk"] = True
            if not new(pick) > OG.BUDGET_K["var"]:
                bad.append(("quarter of a chunk", a, new(pick)))
        dv, dm = w["var"][0, a] - var, w["mean"][0, a] - d["mean"][0, a]
        km = abs(dm) / (U53 * ld["A_mean"][0, a])
        print("DEFECT ds=%d GP %d action variance 1e-3: variance %.3g | %.3g, mean %.3g | %.3g" % (
            ds, a, old(dv), new(dv), abs(dm) / (OG.GPU_MEAN_RTOL * abs(d["mean"][0, a]) + 1e-9), km))
        assert old(dv) <= 1.0 and abs(dm) <= OG.GPU_MEAN_RTOL * abs(d["mean"][0, a]) + 1e-9
        act = max(act, new(dv) / OG.BUDGET_K["var"], km / OG.BUDGET_K["mean"])
    for defect, found in gap.items():
        assert found != ((defect, ds) in NO_GAP), (defect, ds, found)
    if ("action variance", ds) in NOT_SEPARATED:
        print("DEFECT ds=%d action variance: %.3g of the budget -- not separated: %s" % (ds, act, NOT_SEPARATED[("action variance", ds)]))
    elif not act > 1.0:
        bad.append(("action variance", act))
    assert not bad, bad


def _cross_terms(pb, beta, a, b, u, S):
    """beta_a,i beta_b,j E_ij of the cross unit (a, b) (consistent form, oracle/cport/gpmpc_cpu_fullcov.c:129-161), E and the factor c_ab."""
    X, la, lb, sf = pb["X"], pb["lambdas"][a], pb["lambdas"][b], pb["sigma_f"]
    D = X.shape[1]
    V = u - X
    R = S * (1.0 / la + 1.0 / lb)[None, :] + np.eye(D)
    Am = np.linalg.solve(R, S)
    z1, z2 = -V / la, -V / lb
    g1 = -0.5 * (V * V / la).sum(axis=1) + 0.5 * np.einsum("ir,rq,iq->i", z1, Am, z1)
    g2 = -0.5 * (V * V / lb).sum(axis=1) + 0.5 * np.einsum("ir,rq,iq->i", z2, Am, z2)
    E = np.exp(g1[:, None] + g2[None, :] + (z1 @ Am) @ z2.T)
    return sf[a] ** 2 * sf[b] ** 2 / np.sqrt(np.linalg.det(R)), beta[a][:, None] * beta[b][None, :] * E, E


@pytest.mark.parametrize("case", [c for c in OG.FULLCOV_CASES if not c[4]], ids=lambda c: "ds%d-da%d-N%d" % (c[2], c[3], c[1]))
def test_budget_on_the_cross_units(case):
    """Full covariance, every cross unit (a, b).
    swapped weights   the unit summed with the weights of (b, a): beta_b,i beta_a,j under the exponent of (a, b).  With distinct length-scales
                      the exponent is not symmetric in (i, j) and the sums differ -- by 1e3 ... 1e7 project tolerances (printed): a defect the
                      project tolerance already catches at every dimension, so it shows no gap; the budget catches it too (asserted).  (With one
                      lambda the exponent is symmetric and the swap is no defect: those cases are left out.)
    one table step    one pair's term of the unit scaled by 2^(1/2048): the largest pair whose glitch passes the project tolerance on a
                      covariance (1e-4 |cov| + 1e-6 of the largest entry) must miss the budget."""
    from oracle import cport
    cfg, N, ds, da, shared = case
    pb, kinv = OG.problem(cfg, N, ds, da, OG.FULLCOV_H, OG.FULLCOV_B, shared)
    beta, W = cport.constants(pb, kinv)
    u, S = _step2_inputs(pb, beta, W, True)
    d = cport.given_step_full(pb, beta, W, u, S, prec="d", nthreads=THREADS)
    ld = cport.given_step_full(pb, beta, W, u, S, prec="ld", nthreads=THREADS)
    scale = np.abs(d["cov"]).max()
    bad, found = [], False
    for a in range(ds):
        for b in range(a + 1, ds):
            cab, T, E = _cross_terms(pb, beta, a, b, u, S)
            cov, A = d["cov"][0, a, b], ld["A_cov"][0, a, b]
            assert abs(cab * T.sum() - d["mean"][0, a] * d["mean"][0, b] - cov) <= 64.0 * U53 * A       # (numpy's solve and einsum round differently)
            old = lambda dv: np.abs(dv) / (OG.GPU_VAR_RTOL * abs(cov) + 1e-6 * scale)      # noqa: E731
            new = lambda dv: np.abs(dv) / (U53 * A)                                        # noqa: E731
            swap = cab * ((beta[b][:, None] * beta[a][None, :] * E).sum() - T.sum())
            g = cab * np.abs(T).reshape(-1) * TABLE_STEP
            pick = _largest_that_passes(g, old)
            print("DEFECT fullcov ds=%d unit (%d, %d): swapped weights %.3g | %.3g; one table step: of %d pairs the tolerance sees %d, the budget %d, "
                  "the largest pair the tolerance passes: %s" % (ds, a, b, old(swap), new(swap), g.size, (old(g) > 1.0).sum(),
                                                                  (new(g) > OG.BUDGET_K["cov"]).sum(), "none" if pick is None else "%.3g | %.3g" % (old(pick), new(pick))))
            if not new(swap) > OG.BUDGET_K["cov"]:
                bad.append(("swapped weights", a, b, new(swap)))
            if pick is not None:
                found = True
                if not new(pick) > OG.BUDGET_K["cov"]:
                    bad.append(("one table step", a, b, new(pick)))
    assert found != (("cross unit, one table step", ds) in NO_GAP), (ds, found)
    assert not bad, bad
