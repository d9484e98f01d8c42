"""CPU-only tests of the state chance constraints: the float64 reference of tests/constraints_reference.py against finite differences, the
C struct layout, argument validation of the new entry points without a device, StateConstraints, and the cyipopt wiring of
RiskSensitiveMPC (through a stand-in module: cyipopt is not a dependency of the tests).  No GPU compute calls."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

from constraints_reference import reference_constraints
from nominal_reference import synth_nominal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

A3 = np.array([[1.0, 0.0], [0.6, -0.8], [-0.3, 0.5]])       # an axis row, a general row, a mean-only row
B3 = np.array([0.5, 0.2, 0.1])
K3 = np.array([1.6448536269514722, 2.0, 0.0])


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import gaussian_process_mpc_amd as g
    return g


@pytest.mark.parametrize("nominal", [False, True])
def test_reference_jacobian_agrees_with_finite_differences(nominal):
    """The autograd Jacobian of the reference against central differences of the reference's own g (N = 100, ds = 2, da = 2, H = 6,
    three rows: axis, general, kappa = 0; with and without the linear nominal model).

    Step and tolerance from a sweep on this very problem (worst row's relative error | whole matrix, Frobenius, relative):
        h = 1e-1: 1.3e-2 | 3.1e-3     3e-2: 1.1e-3 | 2.8e-4     1e-2: 1.3e-4 | 3.1e-5     3e-3: 1.1e-5 | 2.8e-6
        h = 1e-3: 6.6e-6 | 1.1e-6     3e-4: 1.6e-5 | 3.4e-6     1e-4: 6.1e-5 | 1.1e-5     1e-5: 5.1e-4 | 1.0e-4     1e-6: 5.0e-3 | 9.7e-4
    (the nominal variant: 3.3e-6 | 9.2e-7 at h = 1e-3).  Truncation falls as h^2 down to h = 3e-3; below h = 1e-3 the error grows as
    1 / h, the round-off of the reference's variance (a cancelling sum, ~1e-10 absolute in g).  h = 1e-3 sits at the minimum.  The bounds
    are the project's gradient tolerance for a row, 1e-4 -- what the GPU test holds the kernel to against this reference, 15 x the error
    at the optimum --, and 1e-5 for the whole matrix (9 x)."""
    from gaussian_process_mpc_amd.synth import synth_problem
    from oracle import gpmpc_oracle as O
    H, h = 6, 1e-3
    pb = synth_problem(1, 100, 2, 2, H, 2)
    gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"])
    nom = synth_nominal(2, 2) if nominal else None
    x0, U0 = pb["x0"][0], pb["U"][0].reshape(-1)
    ref = reference_constraints(gp, H, x0, U0, A3, B3, K3, nominal=nom)
    J = ref["jac"]
    assert J.shape == (H * 3, H * 2) and np.all(np.isfinite(J)) and np.all(ref["sd"] > 0)
    for t in range(1, H + 1):                                # causality, exactly
        assert not np.any(J[(t - 1) * 3:t * 3, t * 2:])
        assert np.any(J[(t - 1) * 3:t * 3, (t - 1) * 2:t * 2])
    fd = np.zeros_like(J)
    for c in range(U0.size):
        up, um = U0.copy(), U0.copy()
        up[c] += h
        um[c] -= h
        gp_ = reference_constraints(gp, H, x0, up, A3, B3, K3, nominal=nom, want_jac=False)["g"]
        gm_ = reference_constraints(gp, H, x0, um, A3, B3, K3, nominal=nom, want_jac=False)["g"]
        fd[:, c] = ((gp_ - gm_) / (2 * h)).reshape(-1)
    rows = [np.linalg.norm(fd[i] - J[i]) / np.linalg.norm(J[i]) for i in range(J.shape[0])]
    whole = np.linalg.norm(fd - J) / np.linalg.norm(J)
    print("finite differences, h = %g: worst row %.3e, whole matrix %.3e" % (h, max(rows), whole))
    assert max(rows) <= 1e-4 and whole <= 1e-5


def test_state_constraints_struct_layout_matches_header(built, tmp_path):
    from gaussian_process_mpc_amd._lib import StateConstraintsC, MAX_CONS
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpmpc.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %d",'
                   'sizeof(gpmpc_state_constraints), offsetof(gpmpc_state_constraints,n_rows), offsetof(gpmpc_state_constraints,reserved),'
                   'offsetof(gpmpc_state_constraints,A), offsetof(gpmpc_state_constraints,b), offsetof(gpmpc_state_constraints,kappa),'
                   'GPMPC_MAX_CONS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, o_n, o_res, o_A, o_b, o_k, max_cons = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert size == ctypes.sizeof(StateConstraintsC) and max_cons == MAX_CONS
    assert (o_n, o_res, o_A, o_b, o_k) == (StateConstraintsC.n_rows.offset, StateConstraintsC.reserved.offset, StateConstraintsC.A.offset,
                                           StateConstraintsC.b.offset, StateConstraintsC.kappa.offset)


def test_new_entry_points_validate_arguments_without_a_device(built):
    from gaussian_process_mpc_amd import _lib
    from gaussian_process_mpc_amd._lib import StateConstraintsC, CostParamsC
    lib = built.lib()
    ok = StateConstraintsC()
    ok.n_rows = 2
    fake = ctypes.c_void_p(4096)                             # never dereferenced: every call below is refused before a launch
    pure = lambda c, B=1, H=4, ds=2, da=1, m=fake, v=fake, j=fake, g=fake, gj=fake: lib.gpmpc_rollout_constraints(   # noqa: E731
        B, H, ds, da, None if c is None else ctypes.byref(c), m, v, j, g, gj, None)
    assert pure(None) == -1
    assert pure(ok, m=None) == -1 and pure(ok, v=None) == -1 and pure(ok, g=None) == -1
    assert pure(ok, j=None) == -1                            # a Jacobian output without the step Jacobians
    assert pure(ok, B=0) == -1 and pure(ok, H=0) == -1
    assert pure(ok, ds=0) == -1 and pure(ok, ds=_lib.MAX_DS + 1) == -1 and pure(ok, da=0) == -1 and pure(ok, da=_lib.MAX_D + 1) == -1
    for n in (0, -1, _lib.MAX_CONS + 1):
        bad = StateConstraintsC()
        bad.n_rows = n
        assert pure(bad) == -1
        assert b"n_rows" in lib.gpmpc_last_error()
    for kap in (-1e-300, float("nan"), -float("inf")):
        bad = StateConstraintsC()
        bad.n_rows = 2
        bad.kappa[1] = kap
        assert pure(bad) == -1
        assert b"kappa[1]" in lib.gpmpc_last_error()
    cost = CostParamsC()
    full = lambda p=None, c=ok, flags=1: lib.gpmpc_rollout_constrained(p, 1, 4, fake, fake, ctypes.byref(cost),   # noqa: E731
                                                                       None if c is None else ctypes.byref(c), flags, None, None, fake,
                                                                       fake, fake, fake, fake, 1 << 20, None)
    assert full() == -1                                      # no pack
    assert lib.gpmpc_rollout_constrained_workspace_bytes(None, 1, 4, 1) == 0
    # a pack pointer that is never dereferenced: flags and rows are checked before the pack is looked at
    for flags in (_lib.USE_GRAPH, _lib.WANT_GRAD | _lib.USE_GRAPH, _lib.FP32_ACCUM, _lib.FP32_ALL, 32):
        assert full(fake, flags=flags) == -1
        assert b"GPMPC_WANT_GRAD" in lib.gpmpc_last_error()
        assert lib.gpmpc_rollout_constrained_workspace_bytes(fake, 1, 4, flags) == 0
    assert full(fake, c=None) == -1
    bad = StateConstraintsC()
    bad.n_rows = _lib.MAX_CONS + 1
    assert full(fake, c=bad) == -1 and b"n_rows" in lib.gpmpc_last_error()
    bad.n_rows = 1
    bad.kappa[0] = -0.5
    assert full(fake, c=bad) == -1 and b"kappa[0]" in lib.gpmpc_last_error()


def test_state_constraints_class():
    from gaussian_process_mpc_amd.rollout import StateConstraints
    sc = StateConstraints(A3, B3, kappa=K3)
    assert (sc.m, sc.ds, sc.c.n_rows) == (3, 2, 3)
    np.testing.assert_array_equal(np.array(sc.c.A[:6]).reshape(3, 2), A3)
    np.testing.assert_array_equal(sc.c.b[:3], B3)
    np.testing.assert_array_equal(sc.c.kappa[:3], K3)
    assert not any(sc.c.A[6:]) and not any(sc.c.b[3:]) and not any(sc.c.kappa[3:])
    # prob -> kappa = Phi^-1(prob) = 1.6448536269514722 for 0.95.  statistics.NormalDist().inv_cdf is Wichura's AS241 (PPND16, "about 1
    # part in 10^16"); its last digits depend on the Python version (3.10 returns ...4715, three units in the last place away), so the
    # comparison allows 1e-15 relative -- and the value must be the library function's own, bit for bit
    from statistics import NormalDist
    k95 = StateConstraints([1.0, 0.0], 0.5, prob=0.95).kappa[0]
    assert abs(k95 - 1.6448536269514722) <= 1e-15 * 1.6448536269514722 and k95 == NormalDist().inv_cdf(0.95)
    per_row = StateConstraints(A3, B3, prob=[0.95, 0.5, 0.99])
    np.testing.assert_array_equal(per_row.kappa, [k95, 0.0, NormalDist().inv_cdf(0.99)])
    np.testing.assert_array_equal(StateConstraints(A3, 0.25, kappa=1.5).b, [0.25] * 3)
    np.testing.assert_array_equal(StateConstraints(A3, 0.25, kappa=1.5).kappa, [1.5] * 3)
    # exactly one of the two
    with pytest.raises(ValueError):
        StateConstraints(A3, B3, kappa=K3, prob=0.9)
    with pytest.raises(ValueError):
        StateConstraints(A3, B3)
    for bad in (dict(kappa=-1.0), dict(kappa=float("nan")), dict(prob=0.4), dict(prob=1.0)):
        with pytest.raises(ValueError):
            StateConstraints(A3, B3, **bad)
    with pytest.raises(ValueError):
        StateConstraints(np.ones((17, 2)), 1.0, kappa=0.0)
    with pytest.raises(ValueError):
        StateConstraints(np.ones((2, 9)), 1.0, kappa=0.0)
    # box: upper bounds first, infinite and missing bounds produce no row
    box = StateConstraints.box([None, -8.0, -np.inf], [1.5, 8.0, np.inf], 3, prob=0.95)
    np.testing.assert_array_equal(box.A, [[1, 0, 0], [0, 1, 0], [0, -1, 0]])
    np.testing.assert_array_equal(box.b, [1.5, 8.0, 8.0])
    np.testing.assert_array_equal(box.kappa, [k95] * 3)
    only_ub = StateConstraints.box(None, [np.inf, 2.0], 2, prob=0.9)
    np.testing.assert_array_equal(only_ub.A, [[0, 1]])
    with pytest.raises(ValueError):
        StateConstraints.box([None, None], [np.inf, None], 2, prob=0.9)
    with pytest.raises(ValueError):
        StateConstraints.box([0.0], [1.0], 2, prob=0.9)


class _FakeIpopt(types.ModuleType):
    """Stand-in for the cyipopt module: records Problem(...) and drives the four callbacks once."""

    def __init__(self):
        super().__init__("cyipopt")
        self.calls = []
        outer = self

        class Problem:
            def __init__(self, **kw):
                self.kw = kw
                self.options = {}
                outer.calls.append(self)

            def add_option(self, k, v):
                self.options[k] = v

            def solve(self, x0):
                obj = self.kw["problem_obj"]
                x = np.array(x0, dtype=np.float64)
                self.seen = {"f": obj.objective(x), "df": np.asarray(obj.gradient(x)), "g": obj.constraints(x), "dg": obj.jacobian(x)}
                return x, {}
        self.Problem = Problem


def _bare_mpc(H, ds, da):
    """A RiskSensitiveMPC without a device: only what get_optimal_trajectory and the callbacks touch."""
    import torch
    from gaussian_process_mpc_amd.mpc import RiskSensitiveMPC
    mpc = RiskSensitiveMPC.__new__(RiskSensitiveMPC)
    mpc.horizon, mpc.state_dim, mpc.input_dim = H, ds, da
    mpc.full_covariance, mpc.train_empty, mpc.n_starts = False, False, 1
    mpc.device = torch.device("cpu")
    mpc.last_traj = np.zeros(H * da)
    mpc.lb, mpc.ub = [-1.0] * da, [1.0] * da
    mpc.state_constraints = None
    mpc.curr_g = mpc.curr_g_jac = None
    mpc._cache_key = None
    mpc.solver_used = mpc.last_solve_info = None
    return mpc


def test_cyipopt_wiring_with_and_without_constraints(monkeypatch):
    import gaussian_process_mpc_amd.mpc as M
    fake = _FakeIpopt()
    monkeypatch.setattr(M, "cyipopt", fake)
    monkeypatch.setattr(M, "HAVE_CYIPOPT", True)
    H, ds, da = 5, 2, 2
    mpc = _bare_mpc(H, ds, da)
    evaluated = []

    def stub(x):                                             # what one device pass leaves behind
        evaluated.append(np.array(x))
        mpc.curr_cost, mpc.curr_grad = 1.25, np.full((H, da), 0.5)
        if mpc.state_constraints is not None:
            m = H * mpc.state_constraints.m
            mpc.curr_g = np.arange(m, dtype=np.float64)
            mpc.curr_g_jac = np.arange(m * H * da, dtype=np.float64).reshape(m, H * da)
        return mpc.curr_cost, mpc.curr_grad
    monkeypatch.setattr(mpc, "_evaluate", stub)

    # without constraints: today's arguments and today's callbacks
    U = mpc.get_optimal_trajectory(np.zeros(ds))
    p = fake.calls[-1]
    assert U.shape == (H, da) and mpc.solver_used == "ipopt"
    assert p.kw["m"] == 0 and p.kw["cl"] == [0] and p.kw["cu"] == [0] and p.kw["n"] == H * da and p.kw["problem_obj"] is mpc
    assert p.kw["lb"] == [-1.0] * (H * da) and p.kw["ub"] == [1.0] * (H * da)
    assert p.seen["g"] == 0 and isinstance(p.seen["g"], int)
    assert p.seen["dg"].shape == (H * da,) and not p.seen["dg"].any()
    assert mpc.constraints(np.zeros(H * da)) == 0

    # with constraints: m = H m_c rows, g <= 0, dense row-major Jacobian
    mpc.set_state_constraints(A3, B3, prob=[0.95, 0.9, 0.5])
    m_c = 3
    mpc.get_optimal_trajectory(np.zeros(ds))
    p = fake.calls[-1]
    m = H * m_c
    assert p.kw["m"] == m and p.kw["n"] == H * da
    assert list(p.kw["cu"]) == [0] * m and len(p.kw["cl"]) == m and all(v <= -1e19 for v in p.kw["cl"])
    assert p.seen["g"].shape == (m,) and p.seen["dg"].shape == (m * H * da,) and p.seen["dg"].size == m * H * da
    np.testing.assert_array_equal(p.seen["dg"].reshape(m, H * da)[2], np.arange(2 * H * da, 3 * H * da))       # row-major
    assert p.seen["f"] == 1.25 and p.seen["df"].shape == (H, da)

    # set_state_bounds -> rows of the box; clearing restores the unconstrained problem
    mpc.set_state_bounds([None, -8.0], [None, 8.0], 0.95)
    assert mpc.state_constraints.m == 2
    mpc.get_optimal_trajectory(np.zeros(ds))
    assert fake.calls[-1].kw["m"] == 2 * H
    mpc.clear_state_constraints()
    mpc.get_optimal_trajectory(np.zeros(ds))
    p = fake.calls[-1]
    assert p.kw["m"] == 0 and p.kw["cl"] == [0] and p.kw["cu"] == [0] and p.seen["g"] == 0

    # refusals that need no device
    mpc.set_state_bounds([None, -8.0], [None, 8.0], 0.95)
    with pytest.raises(NotImplementedError, match="multi-start"):
        mpc.get_optimal_trajectory(np.zeros(ds), n_starts=4)
    mpc.full_covariance = True
    with pytest.raises(NotImplementedError, match="full-covariance"):
        mpc.get_optimal_trajectory(np.zeros(ds))
    with pytest.raises(ValueError):
        mpc.set_state_constraints(np.ones((1, 3)), 1.0, kappa=0.0)          # three coefficients for two states


def test_rollout_refuses_graph_and_reduced_precision_with_constraints():
    """Checked before anything touches the device or the pack."""
    from gaussian_process_mpc_amd.rollout import StateConstraints, rollout
    sc = StateConstraints([1.0, 0.0], 1.0, prob=0.9)
    with pytest.raises(ValueError, match="graph"):
        rollout(None, None, None, None, graph=True, constraints=sc)
    with pytest.raises(ValueError, match="precision"):
        rollout(None, None, None, None, want_grad=False, precision="fp32", constraints=sc)
