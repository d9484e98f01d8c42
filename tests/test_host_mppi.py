"""CPU-only tests of the MPPI planner: the numpy restatement of tests/mppi_reference.py (Philox known answers, moments of the normals, every
branch of the update rule, a short run on the pinned oracle), the C struct layout of gpmpc_mppi_params, and the argument validation of the
new entry points without a device.  No GPU compute calls."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mppi_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import gaussian_process_mpc_amd as g
    return g


# ------------------------------------------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,expect", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, expect):
    """The three known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 with 10 rounds)."""
    got = R.philox4x32_10(np.array([counter], dtype=np.uint64), key)[0]
    assert tuple(int(v) for v in got) == expect, [hex(int(v)) for v in got]


def test_normals_moments_and_stream_separation():
    """1 024 000 normals: mean, standard deviation, skewness and kurtosis within 5 / sqrt(n) of 0 / 1 / 0 / 3 (the standard errors are
    1, 0.71, 2.4 and 4.9 over sqrt(n): 5 / sqrt(n) is between 1 and 7 of them)."""
    n = 1024000
    x = R.normals(12345, 0, 0, n)
    m, sd = x.mean(), x.std()
    z = (x - m) / sd
    skew, kurt = (z ** 3).mean(), (z ** 4).mean()
    print("mean %.4f sd %.4f skew %.4f kurtosis %.4f (bound %.4f)" % (m, sd, skew, kurt, 5 / np.sqrt(n)))
    tol = 5 / np.sqrt(n)
    assert abs(m) <= tol and abs(sd - 1) <= tol and abs(skew) <= tol and abs(kurt - 3) <= tol
    # an odd count uses half of the last counter; a prefix of a stream is the stream
    np.testing.assert_array_equal(R.normals(12345, 0, 0, 1001), x[:1001])
    # seed, call index and iteration each give another stream
    for other in (R.normals(12346, 0, 0, 1000), R.normals(12345, 1, 0, 1000), R.normals(12345, 0, 1, 1000), R.normals(12345 + (1 << 32), 0, 0, 1000)):
        assert not np.any(other == x[:1000])


def test_sample_restatement():
    mean = np.linspace(-0.5, 0.5, 15)
    lb, ub = np.array([-0.6, -INF, -0.1]), np.array([0.6, 0.2, INF])
    U = R.sample(mean, 33, 3, [0.5, 1.0, 2.0], lb, ub, seed=7, call_index=2, iteration=3, decay=0.9)
    assert U.shape == (33, 15)
    np.testing.assert_array_equal(U[0], mean)
    j = np.arange(15) % 3
    assert np.all(U[1:] >= lb[j]) and np.all(U[1:] <= ub[j])       # (row 0 is the mean as it came, inside the box or not)
    assert np.any(U[1:, j == 0] == 0.6) and np.any(U[1:, j == 1] == 0.2) and np.any(U[1:, j == 2] == -0.1)        # the bounds bind
    eps = R.normals(7, 2, 3, 33 * 15).reshape(33, 15)
    free = (U > lb[j]) & (U < ub[j])
    free[0] = False
    np.testing.assert_allclose(U[free], (mean[None, :] + np.array([0.5, 1.0, 2.0])[j] * 0.9 ** 3 * eps)[free], rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------------------------------------
# the update rule, branch by branch
# ------------------------------------------------------------------------------------------------------------------------------
U4 = np.array([[1.0, 10.0], [2.0, 20.0], [3.0, 30.0], [4.0, 40.0]])
START = np.array([INF, INF, 0.0, 0.0])


def test_update_unconstrained_softmin():
    cost = np.array([3.0, 1.0, 2.0, 6.0])
    r = R.update(U4, cost, None, np.zeros(2), START, 0.5)
    T = 0.5 * (12.0 / 4 - 1.0)
    w = np.exp(-(cost - 1.0) / T)
    assert r["kstar"] == 1 and r["trace"].tolist() == [0.0, 1.0, 4.0, 4.0, 1.0, T]
    np.testing.assert_allclose(r["mean"], (w[:, None] * U4).sum(0) / w.sum(), rtol=1e-15)
    np.testing.assert_array_equal(r["best"], [0.0, 1.0, 2.0, 20.0])


def test_update_nan_and_infinite_costs():
    cost = np.array([NAN, INF, 2.0, 4.0])
    r = R.update(U4, cost, None, np.zeros(2), START, 1.0)
    # the NaN is dead; the +inf is alive and feasible, has no finite score and no weight
    assert r["trace"].tolist() == [0.0, 2.0, 3.0, 3.0, 2.0, 1.0] and r["kstar"] == 2
    assert r["weights"][0] == 0 and r["weights"][1] == 0 and r["weights"][2] == 1.0
    w3 = np.exp(-2.0)
    np.testing.assert_allclose(r["mean"], (U4[2] + w3 * U4[3]) / (1 + w3), rtol=1e-15)


def test_update_all_dead_leaves_everything():
    best = np.array([0.0, 5.0, 7.0, 8.0])
    r = R.update(U4, np.full(4, NAN), None, np.array([0.25, 0.5]), best, 1.0)
    assert r["trace"].tolist() == [0.0, 5.0, 0.0, 0.0, INF, 0.0] and r["kstar"] is None
    np.testing.assert_array_equal(r["mean"], [0.25, 0.5])
    np.testing.assert_array_equal(r["best"], best)
    g = np.zeros((4, 3))
    g[:, 1] = NAN                                            # dead through the constraints alone
    r = R.update(U4, np.ones(4), g, np.array([0.25, 0.5]), best, 1.0)
    assert r["trace"][3] == 0 and r["kstar"] is None


def test_update_equal_costs_average_the_ties():
    r = R.update(U4, np.full(4, 2.5), None, np.zeros(2), START, 0.3)
    assert r["trace"].tolist() == [0.0, 2.5, 4.0, 4.0, 2.5, 0.0] and r["kstar"] == 0        # T = 0, lowest index
    np.testing.assert_array_equal(r["mean"], U4.mean(axis=0))
    cost = np.array([2.5, 1.0, 1.0, INF])                    # the infinite cost takes no part in the mean of the scores
    r = R.update(U4, cost, None, np.zeros(2), START, 0.3)
    assert r["kstar"] == 1 and r["trace"][5] == 0.5 * 0.3
    r = R.update(U4, np.array([INF, 1.0, INF, 1.0]), None, np.zeros(2), START, 0.3)
    assert r["kstar"] == 1 and r["trace"][5] == 0.0
    np.testing.assert_array_equal(r["mean"], [3.0, 30.0])


def test_update_constraints_feasible_and_restoration():
    cost = np.array([1.0, 2.0, 3.0, 4.0])
    g = np.array([[0.5, -1.0, 0.25], [-1.0, -1.0, -2.0], [0.0, -1.0, 0.125], [-0.5, 0.0, -0.5]])
    r = R.update(U4, cost, g, np.zeros(2), START, 1.0)
    # samples 1 and 3 are feasible (a row at exactly 0 is feasible): only they score, by cost
    assert r["kstar"] == 1 and r["trace"].tolist() == [0.0, 2.0, 2.0, 4.0, 2.0, 1.0]
    assert r["weights"][0] == 0 and r["weights"][2] == 0
    w3 = np.exp(-2.0)
    np.testing.assert_allclose(r["mean"], (U4[1] + w3 * U4[3]) / (1 + w3), rtol=1e-15)
    # exactly one feasible: T = 0, the mean is that sample
    g1 = g.copy()
    g1[3, 1] = 1e-300
    r = R.update(U4, cost, g1, np.zeros(2), START, 1.0)
    assert r["kstar"] == 1 and r["trace"].tolist() == [0.0, 2.0, 1.0, 4.0, 2.0, 0.0]
    np.testing.assert_array_equal(r["mean"], U4[1])
    # none feasible: the score is the violation, the key (v, cost)
    g0 = np.array([[0.5, -1.0, 0.25], [1.0, -1.0, 2.0], [0.0, -1.0, 0.125], [NAN, 0.0, -0.5]])
    r = R.update(U4, cost, g0, np.zeros(2), START, 1.0)
    v = np.array([0.75, 3.0, 0.125])
    T = v.sum() / 3 - 0.125
    assert r["kstar"] == 2 and r["trace"].tolist() == [0.125, 3.0, 0.0, 3.0, 0.125, T]
    np.testing.assert_array_equal(r["best"], [0.125, 3.0, 3.0, 30.0])
    assert r["weights"][3] == 0
    # a feasible key beats any infeasible one, whatever the costs; an infeasible one never replaces a feasible one
    r2 = R.update(U4, cost, g, np.zeros(2), r["best"], 1.0)
    np.testing.assert_array_equal(r2["best"], [0.0, 2.0, 2.0, 20.0])
    r3 = R.update(U4, cost * 0.01, g0, np.zeros(2), r2["best"], 1.0)
    np.testing.assert_array_equal(r3["best"], r2["best"])
    assert r3["trace"][:2].tolist() == [0.0, 2.0]


def test_update_ties_and_strictly_better():
    cost = np.array([2.0, 1.0, 1.0, 3.0])
    r = R.update(U4, cost, None, np.zeros(2), START, 1.0)
    assert r["kstar"] == 1                                   # lowest index of the two
    same = np.array([0.0, 1.0, -7.0, -8.0])                  # an equal key does not replace
    r = R.update(U4, cost, None, np.zeros(2), same, 1.0)
    np.testing.assert_array_equal(r["best"], same)
    worse = np.array([0.0, 0.5, -7.0, -8.0])
    np.testing.assert_array_equal(R.update(U4, cost, None, np.zeros(2), worse, 1.0)["best"], worse)
    better = np.array([0.0, 1.0 + 1e-15, -7.0, -8.0])
    np.testing.assert_array_equal(R.update(U4, cost, None, np.zeros(2), better, 1.0)["best"], [0.0, 1.0, 2.0, 20.0])


def test_fold_order_is_the_documented_one():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(1000) * 10.0 ** rng.integers(-8, 8, 1000)
    p = [0.0] * 256
    for k, v in enumerate(x):
        p[k % 256] = p[k % 256] + v
    h = 128
    while h:
        for i in range(h):
            p[i] = p[i] + p[i + h]
        h //= 2
    assert R._fold(x) == p[0]


# ------------------------------------------------------------------------------------------------------------------------------
# the library: struct layout, refusals without a device
# ------------------------------------------------------------------------------------------------------------------------------
def test_mppi_params_struct_layout_matches_header(built, tmp_path):
    from gaussian_process_mpc_amd._lib import MppiParamsC, MPPI_MAX_SAMPLES
    names = [f[0] for f in MppiParamsC._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpmpc.h"\nint main(){printf("%zu %d"' + ' " %zu"' * len(names)
                   + ', sizeof(gpmpc_mppi_params), GPMPC_MPPI_MAX_SAMPLES, ' + ", ".join("offsetof(gpmpc_mppi_params,%s)" % n for n in names)
                   + ');return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(MppiParamsC) and out[1] == MPPI_MAX_SAMPLES == 4096
    assert out[2:] == [getattr(MppiParamsC, n).offset for n in names]
    assert names == ["n_samples", "iterations", "sigma", "sigma_decay", "beta", "seed", "call_index", "reserved", "lb", "ub"]


def test_mppi_entry_points_validate_arguments_without_a_device(built):
    from gaussian_process_mpc_amd import _lib
    from gaussian_process_mpc_amd._lib import CostParamsC, StateConstraintsC
    from gaussian_process_mpc_amd.mppi import mppi_params
    lib = built.lib()
    fake = ctypes.c_void_p(4096)                             # never dereferenced: every call below is refused before a launch
    good = lambda **kw: mppi_params(**{**dict(samples=8, da=2, sigma=0.5, lb=-1.0, ub=1.0, iterations=3, decay=0.9, beta=0.1), **kw})  # noqa: E731
    smp = lambda P, H=4, ds=2, da=2, it=0, mean=fake, x0=fake, U=fake, xb=fake: lib.gpmpc_mppi_sample(   # noqa: E731
        H, ds, da, None if P is None else ctypes.byref(P), it, mean, x0, U, xb, None)
    assert smp(None) == -1 and smp(good(), mean=None) == -1 and smp(good(), U=None) == -1
    assert smp(good(), x0=None) == -1                        # a batch of start states without the start state
    assert smp(good(), H=0) == -1 and smp(good(), da=0) == -1 and smp(good(), da=_lib.MAX_D + 1) == -1 and smp(good(), ds=_lib.MAX_DS + 1) == -1
    assert smp(good(), it=-1) == -1
    for K in (0, -1, _lib.MPPI_MAX_SAMPLES + 1):
        assert smp(good(samples=K)) == -1 and b"n_samples" in lib.gpmpc_last_error()
    for bad in (0.0, -0.5, NAN):
        assert smp(good(sigma=[0.5, bad])) == -1 and b"sigma[1]" in lib.gpmpc_last_error()
        assert smp(good(decay=bad)) == -1 and b"sigma_decay" in lib.gpmpc_last_error()
        assert smp(good(beta=bad)) == -1 and b"beta" in lib.gpmpc_last_error()
    assert smp(good(lb=[-1.0, 0.5], ub=[1.0, 0.25])) == -1 and b"lb[1]" in lib.gpmpc_last_error()
    assert smp(good(lb=[NAN, 0.0])) == -1 and b"lb[0]" in lib.gpmpc_last_error()

    upd = lambda K=8, H=4, da=2, m=0, beta=0.1, U=fake, c=fake, g=None, mean=fake, bi=fake, bo=ctypes.c_void_p(8192), tr=fake: \
        lib.gpmpc_mppi_update(K, H, da, m, beta, U, c, g, mean, bi, bo, tr, None)   # noqa: E731
    for arg in ("U", "c", "mean", "bi", "bo", "tr"):
        assert upd(**{arg: None}) == -1
    assert upd(K=0) == -1 and upd(K=_lib.MPPI_MAX_SAMPLES + 1) == -1 and upd(H=0) == -1 and upd(da=0) == -1
    assert upd(beta=0.0) == -1 and upd(beta=NAN) == -1
    assert upd(bo=fake) == -1 and b"different buffers" in lib.gpmpc_last_error()
    assert upd(m=2) == -1 and upd(g=fake) == -1 and upd(m=_lib.MAX_CONS + 1, g=fake) == -1 and upd(m=-1) == -1

    cost, P = CostParamsC(), good()
    cons = StateConstraintsC()
    cons.n_rows = 1
    slv = lambda P, p=fake, H=4, cons=None, x0=fake, st=fake, c=cost, oU=fake, ob=fake, tr=fake, ws=fake: lib.gpmpc_mppi_solve(   # noqa: E731
        p, H, x0, st, ctypes.byref(c) if c is not None else None, None if cons is None else ctypes.byref(cons),
        None if P is None else ctypes.byref(P), oU, ob, tr, ws, 1 << 30, None)
    assert slv(P, p=None) == -1 and slv(None) == -1 and slv(P, H=0) == -1 and slv(P, c=None) == -1
    for arg in ("x0", "st", "oU", "ob", "tr", "ws"):
        assert slv(P, **{arg: None}) == -1
    # a pack pointer that is never dereferenced: the scalar parameters and the rows are checked before the pack is looked at
    for K in (0, _lib.MPPI_MAX_SAMPLES + 1):
        assert slv(good(samples=K)) == -1 and b"n_samples" in lib.gpmpc_last_error()
    for iters in (0, -3):
        assert slv(good(iterations=iters)) == -1 and b"iterations" in lib.gpmpc_last_error()
    assert slv(good(beta=-1.0)) == -1 and slv(good(decay=NAN)) == -1
    cons.n_rows = _lib.MAX_CONS + 1
    assert slv(P, cons=cons) == -1 and b"n_rows" in lib.gpmpc_last_error()
    cons.n_rows = 1
    cons.kappa[0] = -1.0
    assert slv(P, cons=cons) == -1 and b"kappa[0]" in lib.gpmpc_last_error()
    assert lib.gpmpc_mppi_solve_workspace_bytes(None, 4, ctypes.byref(P), None) == 0
    assert lib.gpmpc_mppi_solve_workspace_bytes(fake, 4, None, None) == 0
    assert lib.gpmpc_mppi_solve_workspace_bytes(fake, 4, ctypes.byref(good(samples=0)), None) == 0


def test_mpc_refusals_need_no_device():
    import torch
    from gaussian_process_mpc_amd.mpc import RiskSensitiveMPC
    mpc = RiskSensitiveMPC.__new__(RiskSensitiveMPC)
    mpc.horizon, mpc.state_dim, mpc.input_dim = 5, 2, 1
    mpc.full_covariance, mpc.train_empty, mpc.n_starts, mpc.solver = False, False, 1, None
    mpc.device = torch.device("cpu")
    with pytest.raises(ValueError, match="solver"):
        mpc.get_optimal_trajectory(np.zeros(2), solver="cma")
    with pytest.raises(ValueError, match="n_starts"):
        mpc.get_optimal_trajectory(np.zeros(2), solver="mppi", n_starts=4)
    mpc.solver, mpc.n_starts = "mppi", 16
    with pytest.raises(ValueError, match="n_starts"):
        mpc.get_optimal_trajectory(np.zeros(2))
    mpc.n_starts, mpc.full_covariance = 1, True
    with pytest.raises(NotImplementedError, match="full-covariance"):
        mpc.get_optimal_trajectory(np.zeros(2))


# ------------------------------------------------------------------------------------------------------------------------------
# a short run on the oracle
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("constrained", [False, True])
def test_restatement_on_the_oracle_never_loses_its_best(constrained):
    """K = 16, 5 iterations on synth_problem(1, 100, 2, 2, 10, .), trajectory 0, zero start: the best key (violation, cost) never increases,
    the first iteration's slot 0 is the start plan (cost 2.375489), and every iteration's best is at most its slot 0."""
    from gaussian_process_mpc_amd.synth import synth_problem
    from oracle import gpmpc_oracle as O
    pb = synth_problem(1, 100, 2, 2, 10, 64)
    gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"])
    rows = (np.array([[1.0, 0.0]]), np.array([0.35]), np.array([1.6448536269514722])) if constrained else None
    seen = []
    ev = R.oracle_evaluate(gp, 10, pb["x0"][0], pb, 1e-5, rows)

    def evaluate(U):
        c, g = ev(U)
        seen.append((c, g))
        return c, g
    r = R.solve(evaluate, np.zeros(20), 16, 2, 5, 0.5, 0.9, 0.1, 1, 0, -1.0, 1.0)
    tr = r["trace"]
    print(tr)
    assert abs(seen[0][0][0] - 2.375489) < 5e-7
    keys = [(INF, INF)] + [tuple(t[:2]) for t in tr]
    assert all(b <= a for a, b in zip(keys[:-1], keys[1:]))
    assert np.all(np.abs(r["U"]) <= 1.0) and np.all(np.isfinite(tr))
    assert (r["violation"], r["cost"]) == keys[-1]
    if not constrained:
        assert r["cost"] < 2.375489 and np.all(tr[:, 2] == 16)
        assert all(t[1] <= c[0] for t, (c, _) in zip(tr, seen))
