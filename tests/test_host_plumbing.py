"""CPU-only tests of the host plumbing the solvers share: the ORDER of the refusals of the three ``*_solve`` entries (a call with two
faults is refused for the earlier check, with that check's text), and the start points of ``RiskSensitiveMPC._starts``.  No device: the
pointers handed to the library are never dereferenced, every call is refused before the pack is looked at."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import gaussian_process_mpc_amd as g
    return g


FAKE = ctypes.c_void_p(4096)
BIG = 1 << 30


def _refused(lib, rc, text):
    assert rc == -1                                          # GPMPC_E_ARG
    assert lib.gpmpc_last_error() == text.encode()


def _cons(n_rows):
    from gaussian_process_mpc_amd._lib import StateConstraintsC
    c = StateConstraintsC()
    c.n_rows = n_rows
    return c


def test_mppi_solve_refuses_the_scalar_before_the_constraints(built):
    from gaussian_process_mpc_amd._lib import CostParamsC, MAX_CONS
    from gaussian_process_mpc_amd.mppi import mppi_params
    lib, cost = built.lib(), CostParamsC()
    solve = lambda P, cons: lib.gpmpc_mppi_solve(FAKE, 4, FAKE, FAKE, ctypes.byref(cost), ctypes.byref(cons), ctypes.byref(P),  # noqa: E731
                                                 FAKE, FAKE, FAKE, FAKE, BIG, None)
    good = dict(samples=8, da=2, sigma=0.5, lb=-1.0, ub=1.0, iterations=3)
    # each fault on its own, then both: the scalar check runs first
    _refused(lib, solve(mppi_params(**good), _cons(0)), "gpmpc_mppi_solve: n_rows = 0 outside 1..%d" % MAX_CONS)
    _refused(lib, solve(mppi_params(**{**good, "beta": -1.0}), _cons(1)), "gpmpc_mppi_solve: beta = -1 is not positive")
    _refused(lib, solve(mppi_params(**{**good, "beta": -1.0}), _cons(0)), "gpmpc_mppi_solve: beta = -1 is not positive")
    _refused(lib, solve(mppi_params(**{**good, "iterations": 0}), _cons(0)), "gpmpc_mppi_solve: iterations = 0 is less than 1")


def test_auglag_solve_refusal_order(built):
    from gaussian_process_mpc_amd._lib import CostParamsC, MAX_CONS
    from gaussian_process_mpc_amd.device_auglag import auglag_params
    lib, cost = built.lib(), CostParamsC()
    solve = lambda P, cons, first=0, n=2: lib.gpmpc_auglag_solve(FAKE, 4, FAKE, FAKE, ctypes.byref(cost), ctypes.byref(cons),  # noqa: E731
                                                                 ctypes.byref(P), first, n, FAKE, BIG, None)
    good = dict(n_starts=4, da=2, lb=-1.0, ub=1.0)
    who = "gpmpc_auglag_solve: "
    _refused(lib, solve(auglag_params(**good), _cons(0)), who + "n_rows = 0 outside 1..%d" % MAX_CONS)
    _refused(lib, solve(auglag_params(**good), _cons(1), first=-1), who + "first_outer is negative")
    # scalar -> first_outer -> n_outer -> constraints
    _refused(lib, solve(auglag_params(**good, rho0=0.0), _cons(0)), who + "rho0 = 0 is not positive")
    _refused(lib, solve(auglag_params(**good, rho0=0.0), _cons(1), first=-1), who + "rho0 = 0 is not positive")
    _refused(lib, solve(auglag_params(**good, gtol=-1.0), _cons(0), first=-1), who + "gtol = -1 is negative or NaN")      # (the inner search's)
    _refused(lib, solve(auglag_params(**good), _cons(0), first=-1), who + "first_outer is negative")
    _refused(lib, solve(auglag_params(**good), _cons(0), first=-1, n=-1), who + "first_outer is negative")
    _refused(lib, solve(auglag_params(**good), _cons(0), n=-1), who + "n_outer is negative")


def test_lbfgs_solve_refuses_the_scalar_before_the_first_tick(built):
    from gaussian_process_mpc_amd._lib import CostParamsC
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_params
    lib, cost = built.lib(), CostParamsC()
    solve = lambda P, first=0, n=3: lib.gpmpc_lbfgs_solve(FAKE, 4, FAKE, FAKE, ctypes.byref(cost), ctypes.byref(P), first, n,  # noqa: E731
                                                          FAKE, BIG, None)
    good = dict(n_starts=4, da=2, lb=-1.0, ub=1.0)
    who = "gpmpc_lbfgs_solve: "
    _refused(lib, solve(lbfgs_params(**good), first=-1), who + "first_tick is negative")
    _refused(lib, solve(lbfgs_params(**good, gtol=-1.0)), who + "gtol = -1 is negative or NaN")
    _refused(lib, solve(lbfgs_params(**good, gtol=-1.0), first=-1), who + "gtol = -1 is negative or NaN")
    _refused(lib, solve(lbfgs_params(**good, history=0), first=-1, n=-1), who + "history = 0 outside 1..16")
    _refused(lib, solve(lbfgs_params(**good), first=-1, n=-1), who + "first_tick is negative")


def test_starts_are_make_starts_by_hand_and_count_the_solve():
    from gaussian_process_mpc_amd.mpc import RiskSensitiveMPC
    from gaussian_process_mpc_amd.multistart import make_starts
    H, da, K, seed = 5, 2, 6, 11
    mpc = RiskSensitiveMPC.__new__(RiskSensitiveMPC)
    mpc.horizon, mpc.input_dim = H, da
    mpc.solver_used, mpc.last_traj, mpc._solve_count = None, np.zeros(H * da), 0
    lb, ub = H * [-1.0, -2.0], H * [1.0, 0.5]
    opt = {"seed": seed, "spread": 0.7}
    # first solve: no previous plan, no warm start
    X0 = mpc._starts(K, lb, ub, opt)
    want = make_starts(K, H * da, lb, ub, np.random.default_rng([seed, 0]), warm=None, spread=0.7)
    assert X0.shape == (K, H * da) and X0.tobytes() == want.tobytes()
    assert mpc._solve_count == 1
    # second solve: the previous plan shifted by one step, its last input repeated
    plan = np.linspace(-0.9, 0.4, H * da)
    mpc.solver_used, mpc.last_traj = "device-lbfgs x6", plan
    prev = plan.reshape(H, da)
    warm = np.concatenate((prev[1:], prev[-1:]), axis=0).reshape(-1)
    X1 = mpc._starts(K, lb, ub, opt)
    want = make_starts(K, H * da, lb, ub, np.random.default_rng([seed, 1]), warm=warm, spread=0.7)
    assert X1.tobytes() == want.tobytes()
    assert X1.tobytes() != make_starts(K, H * da, lb, ub, np.random.default_rng([seed, 1]), warm=None, spread=0.7).tobytes()
    assert mpc._solve_count == 2
    # warm = False: the previous plan is not used, the solve is counted all the same
    X2 = mpc._starts(K, lb, ub, {**opt, "warm": False})
    assert X2.tobytes() == make_starts(K, H * da, lb, ub, np.random.default_rng([seed, 2]), warm=None, spread=0.7).tobytes()
    assert mpc._solve_count == 3
