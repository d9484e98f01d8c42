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


def ladder_config(ds, da):
    return 40 + 8 * ds + da


def shared_config(ds, da):
    return 140 + 8 * ds + da


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
    for cfg, N, ds, da, H, shared, gamma in (DIAG_CASES[0], DIAG_CASES[2], DIAG_CASES[3]):      # nominal packs, life cycle and class path
        out.append(("case %d N=%d%s" % (cfg, N, " shared" if shared else ""), (cfg, N, ds, da, H, 64, shared), [0, 1, 2, 63], gamma, False))
    for tag, (cfg, N, ds, da, H, shared, gamma) in JAC_CASES.items():
        out.append(("jacobian " + tag, (cfg, N, ds, da, H, 2, shared), [0, 1], gamma, False))
    return out
