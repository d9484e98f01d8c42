"""The CPU checkers OFF the sigma_f = 1 grid (tests/offgrid_problems.py: per-GP amplitudes in [0.6, 1.8], non-zero x_ref / u_ref, coupled Q).

The plain-C ports under oracle/cport use the amplitude where the HIP kernels do (sf^2 in the mean factor, in var = sf^2 - T - mu^2, in the
pair weights) and were pinned to the torch oracle at sigma_f = 1 only (tests/test_oracle_golden.py).  Here they are pinned to the oracle's
autograd on the off-grid inputs, which licenses them as the reference of tests/test_gpu_offgrid.py; and the inputs are shown to discriminate:
a rollout that dropped the amplitudes, or handed each GP a neighbour's, would miss the GPU tolerances by a factor of 100 and more.
No test here needs a GPU.
"""
import numpy as np
import pytest

import offgrid_problems as OG
from oracle import gpmpc_oracle as O

# cport vs oracle: the neighbouring tests' tolerances (test_cport_matches_torch_oracle, test_cport_fullcov_matches_torch_oracle), except where
# the measured deviation exceeds them: then 10 x the measured value (margin for another thread count and libm), and never more than a tenth
# of the GPU tolerance for the same quantity (means 1e-5, variances / covariances 1e-4, cost 1e-6, gradient 1e-4).
DIAG_MEAN_RTOL, DIAG_MEAN_ATOL = 3e-7, 1e-10            # measured 3.0e-8 at N = 200, H = 20 (neighbour: 1e-8)
DIAG_VAR_RTOL = 1e-6
DIAG_COST_RTOL = 1e-8
DIAG_GRAD_RTOL, DIAG_GRAD_ATOL = 1e-6, 1e-9
FC_MEAN_RTOL, FC_MEAN_ATOL = 1e-9, 1e-11
FC_COV_RTOL, FC_COV_ATOL_OF_MAX = 1e-6, 8e-8            # measured 7.8e-9 of the largest entry beyond rtol (neighbour: 1e-9)
FC_COST_RTOL = 1e-9
FC_DDIR_RTOL, FC_DDIR_ATOL = 1e-7, 1e-10
DISCRIMINATION = 100.0                                  # x the GPU tolerance


def _excess(a, b, rtol, atol):
    """max |a - b| / (atol + rtol |b|): what numpy's assert_allclose compares with 1."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (atol + rtol * np.abs(b))))


def _diag_id(c):
    cfg, N, ds, da, H, shared, gamma = c
    return "cfg%d-N%d-ds%d-da%d%s" % (cfg, N, ds, da, "-shared" if shared else "")


def _fullcov_id(c):
    cfg, N, ds, da, shared = c
    return "cfg%d-N%d-ds%d-da%d%s" % (cfg, N, ds, da, "-shared" if shared else "")


# action_dim >= 3 (tests/test_gpu_offgrid.py::test_wide_action_ladder_vs_cport and its long case), in the format of OG.DIAG_CASES
WIDEACT_DIAG = [(OG.wideact_config(ds, da), OG.LADDER_N, ds, da, OG.LADDER_H, False, -1.0) for ds, da in OG.WIDEACT_DIMS] + \
               [OG.WIDEACT_LONG + (False, -1.0)] + [c + (False, -1.0) for c in OG.WIDEACT_MODEL]


@pytest.mark.parametrize("case", OG.DIAG_CASES + WIDEACT_DIAG, ids=_diag_id)
def test_cport_rollout_matches_torch_oracle_off_the_grid(case):
    """cport.rollout (analytic adjoint) against oracle.objective_and_gradient(mode="o2") (autograd), trajectories 0 and B - 1 of B = 4.

    Measured, worst of both trajectories (relative; gradient in norm):
        config  N   ds da H    means    variances  cost     gradient
        1       100 2  2  10   5.9e-10  9.7e-08    8.9e-10  9.9e-10
        2       200 3  1  20   3.0e-08  1.8e-07    1.8e-09  7.4e-10      <- the means exceed the neighbour's 1e-8: rtol 3e-7 = 10 x measured
        3       449 4  1  10   3.1e-10  2.9e-07    3.6e-10  9.9e-10
        3       449 4  1  10   7.0e-10  2.8e-07    5.0e-10  3.6e-10      (one lambda for all GPs)
        4       300 6  1  6    2.0e-10  4.8e-11    5.4e-13  5.8e-12
        3       130 1  1  6    8.5e-11  2.9e-07    3.6e-10  2.6e-10
        5       320 5  2  5    1.2e-10  1.4e-10    2.1e-12  2.6e-12
        7       260 7  1  4    2.0e-13  3.2e-12    3.9e-14  1.9e-13
    The variances deviate by at most 2.9e-7 (inside the neighbour's 1e-6); element by element the gradient stays below 3 % of rtol 1e-6 + atol 1e-9.
    action_dim >= 3 (WIDEACT_DIAG: (ds, da) = (1, 3) ... (5, 3) at N = 150, H = 3; the long case N = 1415, ds = 1, da = 3, H = 2; the H = 4 problems of the
    model tests): means 1.0e-8 and less, variances 6.8e-8 and less, cost 3.2e-10 and less, gradient 6.1e-10 and less; min(1 + gamma Q_kk var) = 0.916.
    The oracle's own trajectories: variances from step 1 on in [1.1e-3, 1.53], min(1 + gamma Q_kk var) = 0.847 -- asserted, not assumed.
    """
    from oracle import cport
    cfg, N, ds, da, H, shared, gamma = case
    B = 4
    pb, kinv = OG.problem(cfg, N, ds, da, H, B, shared)
    assert len(set(pb["sigma_f"])) == ds and pb["sigma_f"].min() >= 0.6 and pb["sigma_f"].max() <= 1.8
    gp = OG.bundle(pb)
    pick = [0, B - 1]
    r = cport.rollout(pb, kinv, gamma, x0=pb["x0"][pick], U=pb["U"][pick], nthreads=4)
    refs = [O.objective_and_gradient(gp, H, pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], gamma, mode="o2") for b in pick]
    for k, o in enumerate(refs):
        OG.assert_diag_reference_is_sane(o["means"], o["vars"], o["cost"], pb["Q"], gamma)
        print("%s [%d]: means %.2e vars %.2e cost %.2e grad %.2e of their tolerances; relative: means %.2e vars %.2e cost %.2e grad (norm) %.2e; "
              "variances from step 1 in [%.3g, %.3g], min(1 + gamma Q var) %.3f" % (
                  _diag_id(case), pick[k], _excess(r["means"][k], o["means"], DIAG_MEAN_RTOL, DIAG_MEAN_ATOL), _excess(r["vars"][k], o["vars"], DIAG_VAR_RTOL, 0.0),
                  _excess(r["cost"][k], o["cost"], DIAG_COST_RTOL, 0.0), _excess(r["grad"][k], o["grad"], DIAG_GRAD_RTOL, DIAG_GRAD_ATOL),
                  _excess(r["means"][k], o["means"], 1.0, DIAG_MEAN_ATOL), _excess(r["vars"][k], o["vars"], 1.0, 0.0), _excess(r["cost"][k], o["cost"], 1.0, 0.0),
                  np.linalg.norm(r["grad"][k] - o["grad"]) / np.linalg.norm(o["grad"]),
                  o["vars"][1:].min(), o["vars"][1:].max(), (1.0 + gamma * np.diag(pb["Q"]) * o["vars"]).min()))
    for k, o in enumerate(refs):                        # (after the print-out: a failing run still shows every figure)
        np.testing.assert_allclose(r["means"][k], o["means"], rtol=DIAG_MEAN_RTOL, atol=DIAG_MEAN_ATOL)
        np.testing.assert_allclose(r["vars"][k], o["vars"], rtol=DIAG_VAR_RTOL)
        np.testing.assert_allclose(r["cost"][k], o["cost"], rtol=DIAG_COST_RTOL)
        np.testing.assert_allclose(r["grad"][k], o["grad"], rtol=DIAG_GRAD_RTOL, atol=DIAG_GRAD_ATOL)


@pytest.mark.parametrize("case", OG.FULLCOV_CASES + OG.WIDEACT_FULLCOV, ids=_fullcov_id)
def test_cport_fullcov_rollout_matches_torch_oracle_off_the_grid(case):
    """cport.rollout_fullcov (complex-step directional derivatives) against oracle.objective_and_gradient_fullcov (autograd): H = 3, both
    trajectories of B = 2, two seeded directions each.

    Measured, worst of both trajectories: means 1.7e-10, cost 6.7e-11, directional derivatives 2.5e-10 relative (all at config 11; the other
    shapes stay below 3e-11 / 4e-12 / 6e-11); covariances 5.0e-8 of the largest entry at config 11 (4.3e-10 and less elsewhere), of which two
    off-diagonal entries of 2.6e-6 lie 7.8e-9 of the largest entry beyond rtol 1e-6 -- more than the neighbour's atol of 1e-9: 8e-8 = 10 x measured,
    below a tenth of the GPU's 1e-6.  Smallest eigenvalue of any covariance 1.0e-3 (the initial one), off-diagonal entries 1-12 % of the largest.
    """
    from oracle import cport
    cfg, N, ds, da, shared = case
    H, B = OG.FULLCOV_H, OG.FULLCOV_B
    pb, kinv = OG.problem(cfg, N, ds, da, H, B, shared)
    gp = OG.bundle(pb)
    dirs = np.random.default_rng(cfg).normal(size=(B, 2, H, da))
    r = cport.rollout_fullcov(pb, kinv, -1.0, dirs=dirs, nthreads=4)
    refs = [O.objective_and_gradient_fullcov(gp, H, pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], -1.0) for b in range(B)]
    for b, o in enumerate(refs):
        OG.assert_fullcov_reference_is_sane(o["means"], o["covs"], o["cost"])
        dd = np.array([float((o["grad"] * dirs[b, d]).sum()) for d in range(2)])
        off = np.abs(o["covs"][1:] * (1.0 - np.eye(ds))).max() / np.abs(o["covs"][1:]).max()
        print("%s [%d]: means %.2e covs %.2e cost %.2e ddir %.2e of their tolerances; relative: means %.2e, covs %.2e of the largest entry, cost %.2e, "
              "ddir %.2e; covs beyond rtol %.2e of the largest entry; smallest eigenvalue %.3g, off-diagonal up to %.3g of the largest entry" % (
                  _fullcov_id(case), b, _excess(r["means"][b], o["means"], FC_MEAN_RTOL, FC_MEAN_ATOL),
                  _excess(r["covs"][b], o["covs"], FC_COV_RTOL, FC_COV_ATOL_OF_MAX * np.abs(o["covs"]).max()), _excess(r["cost"][b], o["cost"], FC_COST_RTOL, 0.0),
                  _excess(r["ddir"][b], dd, FC_DDIR_RTOL, FC_DDIR_ATOL), _excess(r["means"][b], o["means"], 1.0, FC_MEAN_ATOL),
                  np.abs(r["covs"][b] - o["covs"]).max() / np.abs(o["covs"]).max(), _excess(r["cost"][b], o["cost"], 1.0, 0.0),
                  _excess(r["ddir"][b], dd, 1.0, FC_DDIR_ATOL), (np.abs(r["covs"][b] - o["covs"]) - FC_COV_RTOL * np.abs(o["covs"])).max() / np.abs(o["covs"]).max(),
                  np.linalg.eigvalsh(o["covs"]).min(), off))
    for b, o in enumerate(refs):
        np.testing.assert_allclose(r["means"][b], o["means"], rtol=FC_MEAN_RTOL, atol=FC_MEAN_ATOL)
        np.testing.assert_allclose(r["covs"][b], o["covs"], rtol=FC_COV_RTOL, atol=FC_COV_ATOL_OF_MAX * np.abs(o["covs"]).max())
        np.testing.assert_allclose(r["cost"][b], o["cost"], rtol=FC_COST_RTOL)
        for d in range(2):
            np.testing.assert_allclose(r["ddir"][b, d], float((o["grad"] * dirs[b, d]).sum()), rtol=FC_DDIR_RTOL, atol=FC_DDIR_ATOL)


def test_extended_precision_rollout_matches_cport_off_the_grid():
    """cport.rollout_extended (x87 forward pass, its own copy of the amplitude code: oracle/cport/gpmpc_cpu_ld.c) against cport.rollout on the
    N = 300, ds = 6, H = 6 case (six distinct amplitudes), at the tolerances of test_extended_precision_yardstick_matches_reference_fixture
    (means 1e-9, variances 1e-6).  Measured: means 1.8e-10, variances 4.5e-11 relative.
    """
    from oracle import cport
    cfg, N, ds, da, H, shared, gamma = OG.DIAG_CASES[4]
    pb, kinv = OG.problem(cfg, N, ds, da, H, 4, shared)
    e, c = cport.rollout_extended(pb, kinv, nthreads=4), cport.rollout(pb, kinv, gamma, nthreads=4)
    OG.assert_diag_reference_is_sane(c["means"], c["vars"], c["cost"], pb["Q"], gamma)
    print("extended vs fp64 port: means %.2e, variances %.2e relative" % (_excess(c["means"], e["means"], 1.0, 1e-12), _excess(c["vars"], e["vars"], 1.0, 0.0)))
    np.testing.assert_allclose(c["means"], e["means"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(c["vars"], e["vars"], rtol=1e-6)


def _discriminates(label, off, alt, fullcov, what):
    """Trajectory by trajectory: ``alt`` misses the GPU's check against ``off`` by the factor DISCRIMINATION, in the means or in the variances."""
    worst = np.inf
    for k in range(off["means"].shape[0]):
        m = _excess(alt["means"][k], off["means"][k], OG.GPU_MEAN_RTOL, 1e-9)
        if fullcov:
            v = _excess(alt["covs"][k], off["covs"][k], OG.GPU_VAR_RTOL, 1e-6 * np.abs(off["covs"][k]).max())
        else:
            v = _excess(alt["vars"][k], off["vars"][k], OG.GPU_VAR_RTOL, 1e-12)
        worst = min(worst, max(m, v))
    print("%s, %s: every trajectory misses the GPU tolerances by a factor of at least %.3g" % (label, what, worst))
    return worst


_SHAPES = OG.gpu_rollout_shapes()


@pytest.mark.parametrize("shape", _SHAPES, ids=[s[0].replace(" ", "-") for s in _SHAPES])
def test_offgrid_inputs_discriminate(shape):
    """Reference against reference, on every shape and every trajectory tests/test_gpu_offgrid.py compares: the C port's result at the off-grid
    amplitudes differs from its result with sigma_f = 1 for every GP, and (ds >= 2) from its result with the amplitudes handed to the GPs in
    reverse order, by at least 100 x the GPU tolerance (numpy's criterion: |a - b| > 100 (atol + rtol |b|) in some element of the means or of
    the variances / covariances of EVERY trajectory).  A GPU parity test on these inputs cannot pass on a kernel that drops, squares wrongly
    or mis-indexes the amplitude.  A shape that fails here gets another seed, not a smaller factor.

    Measured, the smallest factor over the trajectories of a shape (sigma_f = 1 | reversed): ladder (N = 150, H = 3) ds = 1: 237; ds = 2: 210 | 428;
    ds = 3: 1.3e3 | 2.4e3; ds = 4 ... 7: 6.6e3 and more.  One lambda (N = 150): ds = 2: 138 | 119; ds = 3: 730 | 506; ds = 4, 5: 6.0e3 and more.
    256x128 tiles (N = 520): 512 | 814; balanced runs (N = 2310): above 4.0e3.  Full covariance: ds = 2: 798 | 876; ds = 3 ... 6: 2.3e3 and more.
    Configs 1 / 3 / 3 with one lambda (nominal packs, life cycle, class path): 4.7e3 | 8.4e3, 4.9e3 | 1.3e3, 3.2e3 | 698.  Jacobian cases: 1.9e3 and more.
    action_dim >= 3: ladder (1, 3): 1.1e3; (2, 3): 3.3e3 | 1.9e3; the other dimensions 2.1e3 and more; full covariance 1.7e3 and more; the H = 4 model
    problems 1.4e3 | 471 and 9.4e3 | 1.3e4.  The long case (N = 1415, one GP, H = 2): 117 -- a GP with ten times the data barely feels its amplitude
    (seeds 260 ... 479 give 1.4 ... 324; of the nine above 100, 318, 336, 371 and 472 also keep the double complex floor of
    tests/test_host_accuracy.py within the budget; 472 is taken).  On these shapes also: with x_ref = u_ref = 0 the cost of every trajectory moves by
    1.1e4 ... 4.1e5 x the GPU's cost tolerance, with the coupling of Q dropped (ds >= 2) by 2.1e3 ... 1.0e5.
    """
    from oracle import cport
    label, args, tr, gamma, fullcov = shape
    pb, kinv = OG.problem(*args)
    ds = pb["ds"]
    run = (lambda p, k: cport.rollout_fullcov(p, k, gamma, x0=p["x0"][tr], U=p["U"][tr], nthreads=8)) if fullcov else \
          (lambda p, k: cport.rollout(p, k, gamma, x0=p["x0"][tr], U=p["U"][tr], nthreads=8))
    off = run(pb, kinv)
    if fullcov:
        OG.assert_fullcov_reference_is_sane(off["means"], off["covs"], off["cost"])
    else:
        OG.assert_diag_reference_is_sane(off["means"], off["vars"], off["cost"], pb["Q"], gamma)
    ratios = [_discriminates(label, off, run(*OG.with_sigma_f(pb, np.ones(ds))), fullcov, "sigma_f = 1")]
    if ds >= 2:
        ratios.append(_discriminates(label, off, run(*OG.with_sigma_f(pb, pb["sigma_f"][::-1])), fullcov, "sigma_f reversed"))
    assert min(ratios) >= DISCRIMINATION, (label, ratios)
    if label.startswith("wideact"):
        # the references and the coupling of Q enter the cost alone: back on the grid (x_ref = u_ref = 0; Q diagonal) the cost of every trajectory
        # moves by more than 100 x the GPU's cost tolerance -- a cost kernel that drops u_ref beyond two actions, or the coupling, cannot pass
        for what, q in (("x_ref = u_ref = 0", dict(pb, x_ref=np.zeros(ds), u_ref=np.zeros(pb["da"]))), ("diagonal Q", dict(pb, Q=np.diag(np.diag(pb["Q"]))))):
            if what == "diagonal Q" and ds == 1:
                continue                                    # (one state: Q has no coupling to drop)
            moved = np.abs(run(q, kinv)["cost"] - off["cost"]) / (OG.GPU_COST_RTOL * np.abs(off["cost"]))
            print("%s, %s: the cost of every trajectory moves by at least %.3g x the GPU tolerance" % (label, what, moved.min()))
            assert moved.min() >= DISCRIMINATION, (label, what, moved.min())


@pytest.mark.parametrize("case", [OG.DIAG_CASES[0], OG.DIAG_CASES[2], OG.DIAG_CASES[3]], ids=_diag_id)
def test_offgrid_inputs_discriminate_with_a_nominal_model(case):
    """The same for packs with a linear nominal model, whose GPU reference is tests/nominal_reference.py: its trajectory 0 at the off-grid
    amplitudes against sigma_f = 1 and against the amplitudes reversed, by the criterion of test_offgrid_inputs_discriminate.
    Measured (sigma_f = 1 | reversed): config 1: 4.4e3 | 1.0e4; config 3: 1.0e4 | 1.8e3; config 3 with one lambda: 1.0e5 | 8.4e3."""
    from nominal_reference import assert_reference_is_sane, nominal_rollout, synth_nominal
    cfg, N, ds, da, H, shared, gamma = case
    pb, kinv = OG.problem(cfg, N, ds, da, H, 64, shared)
    W, c = synth_nominal(ds, da)

    def run(p, k):
        gp = O.GPBundle(p["X"], p["Y"], p["lambdas"], p["sigma_f"], p["sigma_n"], Ky_inv=k)
        r = nominal_rollout(gp, W, c, H, p["x0"][0], p["U"][0], p["x_ref"], p["u_ref"], p["Q"], p["R"], gamma, want_grad=False)
        return {"means": r["means"][None], "vars": r["vars"][None], "cost": r["cost"]}

    off = run(pb, kinv)
    assert_reference_is_sane({"means": off["means"][0], "vars": off["vars"][0], "cost": off["cost"]}, pb["Q"], gamma)
    label = "nominal " + _diag_id(case)
    ratios = [_discriminates(label, off, run(*OG.with_sigma_f(pb, np.ones(ds))), False, "sigma_f = 1"),
              _discriminates(label, off, run(*OG.with_sigma_f(pb, pb["sigma_f"][::-1])), False, "sigma_f reversed")]
    assert min(ratios) >= DISCRIMINATION, (label, ratios)
