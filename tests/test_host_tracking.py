"""CPU-only tests of the cost schedule (time-varying references, terminal weight): the float64 reference of tests/tracking_reference.py
against the pinned oracle and against finite differences, the C struct layout, and the refusals of the new entry points that need no
device.  No GPU compute calls."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import tracking_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 6


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import gaussian_process_mpc_amd as g
    return g


@pytest.fixture(scope="module")
def problem():
    from gaussian_process_mpc_amd.synth import synth_problem
    from oracle import gpmpc_oracle as O
    pb = synth_problem(1, 100, 2, 2, H, 2)
    gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"])
    base = T.tracking_objective(gp, H, pb["x0"][0], pb["U"][0], np.zeros((H + 1, 2)), None, pb["Q"], pb["R"], -1.0, want_grad=False)
    Xr, Ur = T.offset_references(base["means"], pb["U"][0], 7)
    return pb, gp, Xr, Ur, T.general_weight(2, 3)


@pytest.mark.parametrize("gamma", [-1.0, 1e-5, 0.0])
@pytest.mark.parametrize("rdelta", [False, True])
def test_constant_schedule_is_the_oracle(problem, gamma, rdelta):
    """A schedule that repeats one x_ref / u_ref, no terminal weight: the reference is oracle.objective_and_gradient's own expression."""
    from oracle import gpmpc_oracle as O
    pb, gp = problem[0], problem[1]
    xr, ur = np.array([0.3, -0.2]), np.array([0.1, -0.4])
    kw = dict(R_delta=0.05 * np.eye(2), last_u=np.array([0.2, -0.1])) if rdelta else {}
    for b in range(2):
        o = O.objective_and_gradient(gp, H, pb["x0"][b], pb["U"][b], xr, ur, pb["Q"], pb["R"], gamma, mode="o2", **kw)
        r = T.tracking_objective(gp, H, pb["x0"][b], pb["U"][b], np.tile(xr, (H + 1, 1)), np.tile(ur, (H, 1)), pb["Q"], pb["R"], gamma, **kw)
        np.testing.assert_allclose(r["cost"], o["cost"], rtol=1e-13)
        np.testing.assert_allclose(r["grad"], o["grad"], rtol=1e-13, atol=1e-16)
        # a terminal weight equal to Q is no terminal weight
        q = T.tracking_objective(gp, H, pb["x0"][b], pb["U"][b], np.tile(xr, (H + 1, 1)), np.tile(ur, (H, 1)), pb["Q"], pb["R"], gamma,
                                 Q_terminal=pb["Q"], **kw)
        np.testing.assert_allclose(q["cost"], o["cost"], rtol=1e-13)


@pytest.mark.parametrize("fullcov", [False, True])
def test_constant_schedule_is_the_fullcov_oracle_too(problem, fullcov):
    from oracle import gpmpc_oracle as O
    pb, gp = problem[0], problem[1]
    xr, ur = np.array([0.3, -0.2]), np.array([0.1, -0.4])
    f = O.objective_and_gradient_fullcov if fullcov else (lambda *a, **k: O.objective_and_gradient(*a, mode="o2", **k))
    o = f(gp, 3, pb["x0"][0], pb["U"][0][:3], xr, ur, pb["Q"], pb["R"], -1.0)
    r = T.tracking_objective(gp, 3, pb["x0"][0], pb["U"][0][:3], np.tile(xr, (4, 1)), np.tile(ur, (3, 1)), pb["Q"], pb["R"], -1.0, fullcov=fullcov)
    np.testing.assert_allclose(r["cost"], o["cost"], rtol=1e-13)
    np.testing.assert_allclose(r["grad"], o["grad"], rtol=1e-13, atol=1e-16)


@pytest.mark.parametrize("gamma", [-1.0, 1e-5, 0.0])
def test_reference_gradient_agrees_with_finite_differences(problem, gamma):
    """The autograd gradient of the tracking reference against central differences of its own cost (N = 100, ds = 2, da = 2, H = 6,
    references offset from the plan by O(1) -- cost 0.97 --, a non-symmetric terminal weight, input references on).

    Step and tolerance from a sweep on this very problem (error of the whole gradient in norm, relative; gamma = -1 | 1e-5 | 0):
        h = 1e-1: 8.1e-4 | 7.7e-4 | 7.7e-4     3e-2: 7.2e-5 | 6.9e-5 | 6.9e-5     1e-2: 8.0e-6 | 7.7e-6 | 7.6e-6
        h = 3e-3: 7.3e-7 | 7.3e-7 | 7.0e-7     1e-3: 2.0e-7 | 2.3e-7 | 1.9e-7     3e-4: 4.6e-7 | 9.2e-7 | 4.3e-7
        h = 1e-4: 1.8e-6 | 3.2e-6 | 1.7e-6     1e-5: 1.6e-5 | 3.4e-5 | 1.5e-5     1e-6: 1.4e-4 | 2.8e-4 | 1.3e-4
    Truncation falls as h^2 down to h = 3e-3; below h = 1e-3 the error grows as 1 / h (round-off of the variance, a cancelling sum).
    h = 1e-3 sits at the minimum; the bound is 1e-5, a tenth of the project's gradient tolerance -- what the GPU test holds the kernels
    to against this reference -- and 40 x the error at the optimum."""
    pb, gp, Xr, Ur, Qf = problem
    h, x0, U0 = 1e-3, pb["x0"][0], pb["U"][0].reshape(-1)
    kw = dict(Q_terminal=Qf)
    ref = T.tracking_objective(gp, H, x0, U0, Xr, Ur, pb["Q"], pb["R"], gamma, **kw)
    assert np.isfinite(ref["cost"]) and 0.1 < ref["cost"] < 10.0
    fd = np.zeros(U0.size)
    for c in range(U0.size):
        up, um = U0.copy(), U0.copy()
        up[c] += h
        um[c] -= h
        fd[c] = (T.tracking_objective(gp, H, x0, up, Xr, Ur, pb["Q"], pb["R"], gamma, want_grad=False, **kw)["cost"]
                 - T.tracking_objective(gp, H, x0, um, Xr, Ur, pb["Q"], pb["R"], gamma, want_grad=False, **kw)["cost"]) / (2 * h)
    g = ref["grad"].reshape(-1)
    err = np.linalg.norm(fd - g) / np.linalg.norm(g)
    print("finite differences, gamma = %g, h = %g: %.3e" % (gamma, h, err))
    assert err <= 1e-5


@pytest.mark.parametrize("gamma", [-1.0, 0.0])
def test_additivity_one_row_changes_one_term(problem, gamma):
    """Changing only row t* of X_ref changes the cost by exactly that step's term (and the last row is the one under Q_terminal)."""
    pb, gp, Xr, Ur, Qf = problem
    x0, U0 = pb["x0"][0], pb["U"][0]
    a = T.tracking_objective(gp, H, x0, U0, Xr, Ur, pb["Q"], pb["R"], gamma, Q_terminal=Qf, want_grad=False)
    for ts in (0, 3, H):
        X2 = Xr.copy()
        X2[ts] += np.array([0.25, -0.5])
        b = T.tracking_objective(gp, H, x0, U0, X2, Ur, pb["Q"], pb["R"], gamma, Q_terminal=Qf, want_grad=False)
        same = [i for i in range(H + 1) if i != ts]
        assert [a["terms"][i] for i in same] == [b["terms"][i] for i in same]
        assert a["terms"][ts] != b["terms"][ts]
        np.testing.assert_allclose(b["cost"] - a["cost"], b["terms"][ts] - a["terms"][ts], rtol=1e-12, atol=1e-15)
    # the terminal weight reaches the last term only
    c = T.tracking_objective(gp, H, x0, U0, Xr, Ur, pb["Q"], pb["R"], gamma, want_grad=False)
    assert c["terms"][:H] == a["terms"][:H] and c["terms"][H] != a["terms"][H]


def test_cost_params_keep_their_layout_and_schedule_id_replaces_reserved(built, tmp_path):
    from gaussian_process_mpc_amd._lib import CostParamsC, MAX_D, MAX_DS
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpmpc.h"\nint main(){printf("%zu %zu %zu %zu %zu",'
                   'sizeof(gpmpc_cost_params), offsetof(gpmpc_cost_params,R), offsetof(gpmpc_cost_params,x_ref),'
                   'offsetof(gpmpc_cost_params,has_R_delta), offsetof(gpmpc_cost_params,schedule_id));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off_R, off_xref, off_flag, off_id = (int(v) for v in subprocess.check_output([str(exe)]).split())
    # the numbers of the struct before the schedule: 1 + 64 + 3 * 64 + 8 + 8 + 8 doubles, then two ints
    n_d = 1 + MAX_DS * MAX_DS + 2 * MAX_D * MAX_D + MAX_DS + 2 * MAX_D
    assert size == 8 * n_d + 8 == ctypes.sizeof(CostParamsC)
    assert off_R == 8 * (1 + MAX_DS * MAX_DS) == CostParamsC.R.offset
    assert off_xref == 8 * (1 + MAX_DS * MAX_DS + 2 * MAX_D * MAX_D) == CostParamsC.x_ref.offset
    assert off_flag == 8 * n_d == CostParamsC.has_R_delta.offset
    assert off_id == 8 * n_d + 4 == CostParamsC.schedule_id.offset        # where `reserved` sat
    assert CostParamsC().schedule_id == 0                                   # a zero-filled struct has no schedule


def test_schedule_entry_points_refuse_without_a_device(built):
    from gaussian_process_mpc_amd import _lib
    from gaussian_process_mpc_amd._lib import CostParamsC
    lib = built.lib()
    out = ctypes.c_int(-7)
    for args in ((0, 2, 1), (-1, 2, 1), (4, 0, 1), (4, _lib.MAX_DS + 1, 1), (4, 2, -1), (4, 2, _lib.MAX_D + 1)):
        assert lib.gpmpc_cost_schedule_create(*args, ctypes.byref(out)) == -1 and out.value == -7
    assert lib.gpmpc_cost_schedule_create(4, 2, 1, None) == -1
    x = (ctypes.c_double * 16)()
    for bad in (1, 12345, -3):                                              # no schedule was ever created in this process
        assert lib.gpmpc_cost_schedule_destroy(bad) == -1 and b"unknown or destroyed" in lib.gpmpc_last_error()
        assert lib.gpmpc_cost_schedule_set(bad, 2, x, None, None, None) == -1 and b"unknown or destroyed" in lib.gpmpc_last_error()
        assert lib.gpmpc_cost_schedule_set_dev(bad, 2, ctypes.c_void_p(4096), None, None, None) == -1
        assert b"unknown or destroyed" in lib.gpmpc_last_error()
        assert lib.gpmpc_cost_schedule_get(bad, None, None, None, None, None, None) == -1
    assert lib.gpmpc_cost_schedule_set(1, 2, None, None, None, None) == -1 and b"x_ref" in lib.gpmpc_last_error()
    # a cost that names an unknown schedule is refused before anything is looked at on the device (pointers never dereferenced)
    fake = ctypes.c_void_p(4096)
    cost = CostParamsC()
    cost.schedule_id = 77
    assert lib.gpmpc_cost(1, 4, 2, 1, ctypes.byref(cost), fake, fake, fake, fake, None) == -1
    assert b"cost schedule 77 is unknown or destroyed" in lib.gpmpc_last_error()
    assert lib.gpmpc_cost_grad(1, 4, 2, 1, ctypes.byref(cost), fake, fake, fake, fake, fake, fake, fake, None) == -1
    assert b"gpmpc_cost" in lib.gpmpc_last_error()


def test_signatures_cover_the_schedule_entries(built):
    from gaussian_process_mpc_amd import _lib
    for name in ("gpmpc_cost_schedule_create", "gpmpc_cost_schedule_destroy", "gpmpc_cost_schedule_set", "gpmpc_cost_schedule_set_dev",
                 "gpmpc_cost_schedule_get"):
        assert name in _lib.SIGNATURES and getattr(built.lib(), name)
    assert [f[0] for f in _lib.CostParamsC._fields_][-2:] == ["has_R_delta", "schedule_id"]
