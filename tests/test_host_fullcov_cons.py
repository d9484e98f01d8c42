"""Holds tests/fullcov_cons_reference.py itself and everything of the chance constraints under the full covariance that needs no device (CPU):

  * the reference is sane on the cases the GPU test uses (those of tests/test_gpu_constraints.py, plans 0 and 1): every radicand
    a^T Sigma_t a is positive and every Sigma_t positive definite, so every row is on the differentiable branch;
  * it DISCRIMINATES: the diagonal rule (q = sum a_k^2 var_k) misses the tolerance the GPU test holds g to by at least 50 times on the general
    kappa = 2 row of every case -- a test against the full rule cannot pass on the diagonal code;
  * the packing rule of k_fc_pack_jac, restated in numpy (``pack_jacobian``), reproduces a dense chain-rule product on random inputs whose
    stored d/dS is NOT symmetrised: this pins "an off-diagonal Sigma_kl is ONE variable, its column is d/dS_kl + d/dS_lk";
  * the C ABI: names, declarations, argument counts, exports, the Python keywords, and the refusals that need no pack.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fullcov_cons_reference as F
import test_gpu_constraints as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ("c1", "c2", "c3", "c3s", "d6")
NAMES = ("gpmpc_rollout_fullcov_jac", "gpmpc_rollout_fullcov_jac_workspace_bytes", "gpmpc_rollout_fullcov_constrained",
         "gpmpc_rollout_fullcov_constrained_workspace_bytes", "gpmpc_mppi_solve_fullcov", "gpmpc_mppi_solve_fullcov_workspace_bytes",
         "gpmpc_lbfgs_solve_fullcov", "gpmpc_lbfgs_solve_fullcov_workspace_bytes", "gpmpc_auglag_solve_fullcov",
         "gpmpc_auglag_solve_fullcov_workspace_bytes")
_fwd = {}


def forward_ref(tag, b):
    """The reference without its Jacobian (a forward pass of the oracle), computed once."""
    if (tag, b) not in _fwd:
        pb, gp = TC._problem(tag)
        A, bb, kap = TC._rows(pb["ds"])
        _fwd[(tag, b)] = F.reference_fullcov_constraints(gp, pb["H"], pb["x0"][b], pb["U"][b], A, bb, kap, want_jac=False)
    return _fwd[(tag, b)]


@pytest.mark.parametrize("tag", TAGS)
def test_reference_is_on_the_differentiable_branch(tag):
    for b in (0, 1):
        ref = forward_ref(tag, b)
        eig = np.linalg.eigvalsh(ref["covs"])
        print("  %s [%d]: smallest a^T Sigma a %.3e, smallest eigenvalue of a Sigma_t %.3e" % (tag, b, ref["q"].min(), eig.min()))
        assert np.all(np.isfinite(ref["g"])) and ref["q"].min() > 0.0 and eig.min() > 0.0
        assert np.abs(ref["covs"] - np.swapaxes(ref["covs"], 1, 2)).max() == 0.0


@pytest.mark.parametrize("tag", TAGS)
def test_reference_discriminates_the_diagonal_rule(tag):
    A, _, kap = TC._rows(TC.CASES[tag][2])
    assert kap[1] == 2.0 and np.count_nonzero(A[1]) > 1
    for b in (0, 1):
        ref = forward_ref(tag, b)
        ratio = np.abs(ref["g_diag"] - ref["g"]) / F.g_tolerance(ref, A, kap)
        print("  %s [%d]: the diagonal rule misses the tolerance of the kappa = 2 row by x%.0f (largest), x%.1f (smallest step)"
              % (tag, b, ratio[:, 1].max(), ratio[:, 1].min()))
        assert ratio[:, 1].max() >= 50.0
        # the mean-only row (kappa = 0) does not see the covariance and the off-diagonals do not enter the axis row a = e_0: there both
        # rules agree up to the rounding of two ways of summing
        assert ratio[:, 2].max() <= 1e-3 and ratio[:, 0].max() <= 1e-3


def test_batched_rows_are_the_rows_of_the_loop():
    """The reference's Jacobian by one batched autograd call against one call per row (c1, plan 0): the same backward passes, vectorised --
    they agree far inside the 1e-4 of the gradient criterion (measured: 9e-10 relative on c2, where the oracle's explicit inverses amplify the
    order of the sums most)."""
    pb, gp = TC._problem("c1")
    A, bb, kap = TC._rows(pb["ds"])
    one = F.reference_fullcov_constraints(gp, pb["H"], pb["x0"][0], pb["U"][0], A, bb, kap, batched=False)
    all_ = F.reference_fullcov_constraints(gp, pb["H"], pb["x0"][0], pb["U"][0], A, bb, kap)
    assert one["jac"].shape == all_["jac"].shape == (pb["H"] * 3, pb["H"] * pb["da"]) and np.array_equal(one["g"], all_["g"])
    rel = np.abs(one["jac"] - all_["jac"]).max() / np.abs(one["jac"]).max()
    print("  c1: batched rows against the loop: %.3e relative to the largest entry" % rel)
    assert rel <= 1e-8
    for t in range(1, pb["H"] + 1):                          # causality, exactly, in both
        assert not np.any(one["jac"][(t - 1) * 3:t * 3, t * pb["da"]:]) and not np.any(all_["jac"][(t - 1) * 3:t * 3, t * pb["da"]:])


@pytest.mark.parametrize("tag", TAGS)
def test_batched_rows_on_every_case(tag):
    """The form the GPU test relies on, on each of its cases (plan 0): rows of the batched Jacobian -- the first, the last and two in between,
    which fall into different batches where a case has several -- against ``torch.autograd.grad`` on that row alone.  Bound: 1e-6 of the
    row's norm, a hundredth of the gradient criterion the rows serve (both are float64 backward passes over one graph; they differ by
    the order of sums that the oracle's explicit inverses amplify: measured 9e-10 on c2)."""
    pb, gp = TC._problem(tag)
    A, bb, kap = TC._rows(pb["ds"])
    R = pb["H"] * 3
    rows = sorted({0, R // 3, (2 * R) // 3 + 1, R - 1})
    full = F.reference_fullcov_constraints(gp, pb["H"], pb["x0"][0], pb["U"][0], A, bb, kap)
    loop = F.reference_fullcov_constraints(gp, pb["H"], pb["x0"][0], pb["U"][0], A, bb, kap, batched=False, only_rows=rows)
    assert loop["jac"].shape == (len(rows), pb["H"] * pb["da"])
    rel = [np.linalg.norm(full["jac"][i] - loop["jac"][k]) / np.linalg.norm(loop["jac"][k]) for k, i in enumerate(rows)]
    print("  %s: batched rows %s against the loop, relative error in norm: %s" % (tag, rows, " ".join("%.2e" % v for v in rel)))
    assert max(rel) <= 1e-6


def test_g_tolerance_is_the_covariance_tolerance_pushed_through():
    """One step, one row, by hand."""
    mu, S = np.array([[0.0, 0.0], [0.3, -0.2]]), np.array([np.eye(2), [[0.04, 0.01], [0.01, 0.09]]])
    A, kap = np.array([[1.0, -2.0]]), np.array([2.0])
    q = 0.04 - 4 * 0.01 + 4 * 0.09
    ref = {"means": mu, "covs": S, "sd": np.array([[np.sqrt(q)]])}
    dq = (1e-4 * 0.04 + 1e-6 * 0.09) + 2 * 2 * (1e-4 * 0.01 + 1e-6 * 0.09) + 4 * (1e-4 * 0.09 + 1e-6 * 0.09)
    want = 1e-5 * (0.3 + 0.4) + 2.0 * dq / (2 * np.sqrt(q)) + 1e-9
    np.testing.assert_allclose(F.g_tolerance(ref, A, kap), [[want]], rtol=1e-13)


# ------------------------------------------------------------------------------------------------------------------ the packing rule
def _dense(dmu_du, dmu_dS, dc_du, dc_dS, ds, da):
    """The step Jacobian over the UNPACKED state (mu (ds), vec Sigma (ds^2), u (da)): rows (mu', vec Sigma')."""
    D = ds + da
    n = ds + ds * ds
    M = np.zeros((n, n + da))
    M[:ds, :ds] = dmu_du[:, :ds]
    M[:ds, ds:n] = dmu_dS[:, :ds, :ds].reshape(ds, ds * ds)
    M[:ds, n:] = dmu_du[:, ds:]
    M[ds:, :ds] = dc_du.reshape(ds * ds, D)[:, :ds]
    M[ds:, ds:n] = dc_dS[:, :, :ds, :ds].reshape(ds * ds, ds * ds)
    M[ds:, n:] = dc_du.reshape(ds * ds, D)[:, ds:]
    return M


@pytest.mark.parametrize("ds,da", [(1, 1), (2, 2), (3, 1), (6, 2)])
def test_packing_rule_reproduces_the_dense_chain_rule(ds, da):
    rng = np.random.default_rng(100 * ds + da)
    D, tri = ds + da, F.tri_pairs(ds)
    nt, p = len(tri), ds + len(tri)
    # E: packed symmetric variable -> vec Sigma (both entries of an off-diagonal); Rm: vec Sigma' -> its upper triangle
    E, Rm = np.zeros((ds * ds, nt)), np.zeros((nt, ds * ds))
    for c, (k, l) in enumerate(tri):
        E[k * ds + l, c] = E[l * ds + k, c] = 1.0
        Rm[c, k * ds + l] = 1.0
    up = np.block([[np.eye(ds), np.zeros((ds, nt))], [np.zeros((ds * ds, ds)), E]])                    # packed state -> unpacked
    down = np.block([[np.eye(ds), np.zeros((ds, ds * ds))], [np.zeros((nt, ds)), Rm]])                 # unpacked -> packed
    steps = []
    for _ in range(3):
        dmu_du, dmu_dS = rng.standard_normal((ds, D)), rng.standard_normal((ds, D, D))                 # d/dS NOT symmetrised
        dc_du, dc_dS = rng.standard_normal((ds, ds, D)), rng.standard_normal((ds, ds, D, D))
        dc_du, dc_dS = dc_du + dc_du.transpose(1, 0, 2), dc_dS + dc_dS.transpose(1, 0, 2, 3)           # Sigma' is symmetric: rows (a, b) = (b, a)
        steps.append((dmu_du, dmu_dS, dc_du, dc_dS))
    packed = [F.pack_jacobian(*s, ds, da) for s in steps]
    dense = [_dense(*s, ds, da) for s in steps]
    n = ds + ds * ds
    for J, M in zip(packed, dense):
        assert J.shape == (p, p + da)
        # one step: a symmetric perturbation through the dense map, packed, is the packed map of the packed perturbation
        want = np.block([down @ M[:, :n] @ up, down @ M[:, n:]])
        np.testing.assert_allclose(J, want, rtol=0, atol=1e-14 * np.abs(want).max())
    # three steps: d(state_3) / d(u_0) by the dense chain rule, packed, against the chain of packed Jacobians
    chain_dense = down @ dense[2][:, :n] @ dense[1][:, :n] @ dense[0][:, n:]
    chain_packed = packed[2][:, :p] @ packed[1][:, :p] @ packed[0][:, p:]
    np.testing.assert_allclose(chain_packed, chain_dense, rtol=0, atol=1e-13 * np.abs(chain_dense).max())
    if ds > 1:
        # ... and "2 x one entry" in the place of the sum is a different matrix on these inputs
        k, l = tri[1]
        wrong = packed[0].copy()
        wrong[:ds, ds + 1] = 2.0 * steps[0][1][:, k, l]
        assert np.abs(wrong - packed[0]).max() > 1e-3


# ------------------------------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_mpc_amd import _lib
    return _lib.lib()


def test_abi_names_signatures_and_exports(L):
    from gaussian_process_mpc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    assert "Full-covariance rollout: Jacobian and chance constraints" in hdr and "d/dS_kl + d/dS_lk" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_size_t if name.endswith("_bytes") else ctypes.c_int)
        assert getattr(L, name) is not None
        n_decl = len(re.search(r"\b%s\s*\((.*?)\);" % name, hdr, flags=re.S).group(1).split(","))
        assert n_decl == len(args), (name, n_decl, len(args))
    # a new solver entry takes what its sibling takes
    for new, old in (("gpmpc_mppi_solve_fullcov", "gpmpc_mppi_solve"), ("gpmpc_lbfgs_solve_fullcov", "gpmpc_lbfgs_solve"),
                     ("gpmpc_auglag_solve_fullcov", "gpmpc_auglag_solve"), ("gpmpc_rollout_fullcov_constrained", "gpmpc_rollout_constrained")):
        assert _lib.SIGNATURES[new] == _lib.SIGNATURES[old]
        assert _lib.SIGNATURES[new + "_workspace_bytes"] == _lib.SIGNATURES[old + "_workspace_bytes"]
    import gaussian_process_mpc_amd as g
    assert hasattr(g, "rollout_fullcov_jac") and "rollout_fullcov_jac" in g.__all__
    assert inspect.signature(g.rollout_fullcov).parameters["constraints"].default is None
    for fn in (g.mppi_solve, g.lbfgs_solve, g.lbfgs_tick, g.auglag_solve):
        assert inspect.signature(fn).parameters["full_covariance"].default is False
    assert g.RiskSensitiveMPC.propagation == "moment_matching"


def test_refusals_that_need_no_pack(L):
    """NULL arguments are GPMPC_E_ARG and the size queries of a NULL pack 0, without a device."""
    from gaussian_process_mpc_amd._lib import AuglagParamsC, CostParamsC, LbfgsParamsC, MppiParamsC, StateConstraintsC
    p = ctypes.c_void_p
    a = p(0x2000)
    cost, cons = CostParamsC(), StateConstraintsC()
    cons.n_rows = 1
    assert L.gpmpc_rollout_fullcov_jac(None, 1, 2, a, a, a, a, a, a, 1 << 20, None) == -1
    assert L.gpmpc_rollout_fullcov_constrained(None, 1, 2, a, a, ctypes.byref(cost), ctypes.byref(cons), 0, None, None, a, None, a, None, a,
                                               1 << 20, None) == -1
    assert L.gpmpc_rollout_fullcov_jac_workspace_bytes(None, 1, 2) == 0
    assert L.gpmpc_rollout_fullcov_constrained_workspace_bytes(None, 1, 2, 0) == 0
    mp, lp, ap = MppiParamsC(), LbfgsParamsC(), AuglagParamsC()
    mp.n_samples, lp.n_starts, lp.history = 4, 2, 4
    ap.inner = lp
    assert L.gpmpc_mppi_solve_fullcov_workspace_bytes(None, 2, ctypes.byref(mp), None) == 0
    assert L.gpmpc_lbfgs_solve_fullcov_workspace_bytes(None, 2, ctypes.byref(lp)) == 0
    assert L.gpmpc_auglag_solve_fullcov_workspace_bytes(None, 2, ctypes.byref(cons), ctypes.byref(ap)) == 0
    assert L.gpmpc_mppi_solve_fullcov(None, 2, a, a, ctypes.byref(cost), None, ctypes.byref(mp), a, a, a, a, 1 << 20, None) == -1
    assert L.gpmpc_lbfgs_solve_fullcov(None, 2, a, a, ctypes.byref(cost), ctypes.byref(lp), 0, 1, a, 1 << 20, None) == -1
    assert L.gpmpc_auglag_solve_fullcov(None, 2, a, a, ctypes.byref(cost), ctypes.byref(cons), ctypes.byref(ap), 0, 1, a, 1 << 20, None) == -1
