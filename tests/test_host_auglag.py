"""CPU-only tests of the constrained multi-start: the numpy restatement of tests/auglag_reference.py -- its merit gradient
against central differences, the rule on a small convex problem with a known KKT point, the rule on the pinned oracle for c1 --, the C struct
layout and the state-buffer arithmetic, the argument validation of the new entry points without a device, the solver= handling of
RiskSensitiveMPC.  No GPU compute calls."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import auglag_reference as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
K95 = 1.6448536269514722


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import gaussian_process_mpc_amd as g
    return g


# ------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------------------
def _analytic(X):
    """f = sum_c cos(x_c) + 0.5 |x|^2 w, g_i = sin(a_i . x) + 0.1 |x|^2 - b_i: smooth, with dense Jacobians; R = 6 rows, n = 5."""
    rng = np.random.default_rng(3)
    n = X.shape[1]
    w = rng.uniform(0.5, 2.0, n)
    A = rng.standard_normal((6, n))
    b = np.array([0.9, -0.2, 0.3, 1.5, -0.6, 0.0])
    f = np.cos(X).sum(axis=1) + 0.5 * (X * X * w).sum(axis=1)
    grad = -np.sin(X) + X * w
    z = X @ A.T
    g = np.sin(z) + 0.1 * (X * X).sum(axis=1)[:, None] - b
    g_jac = np.cos(z)[:, :, None] * A[None, :, :] + 0.2 * X[:, None, :]
    return f, grad, g, g_jac


def test_merit_gradient_against_central_differences():
    """dM against (M(x + h e_c) - M(x - h e_c)) / 2h on the analytic (f, g) above, K = 4 points, rows active and inactive at every point,
    no row within 1e-3 of the switch t_i = 0 (asserted: M is C1 but not C2 there).  Sweep of h on these inputs, largest error relative to
    max |dM|: h = 1e-3: 1.5e-6, 1e-4: 1.5e-8, 1e-5: 1.7e-10, 1e-6: 1.6e-10, 1e-7: 1.1e-9 -- truncation ~ h^2 down to 1e-5, rounding ~ eps / h
    from 1e-6 on.  The test uses h = 1e-5 and a tolerance of 1e-9: 6 x the truncation error the h^2 law predicts there (1.5e-10), and 15 x
    below what the next larger step gives."""
    rng = np.random.default_rng(0)
    K, n = 4, 5
    X = rng.uniform(-1, 1, (K, n))
    lam = rng.uniform(0, 2, (K, 6)) * (rng.uniform(size=(K, 6)) < 0.6)
    rho = np.array([0.5, 10.0, 3.0, 100.0])
    f, grad, g, g_jac = _analytic(X)
    psi, t = AR.psi_of(g, lam, rho)
    assert np.abs(t).min() > 1e-3 and (psi > 0).any(axis=1).all() and (psi == 0).any(axis=1).all()
    M, dM = AR.merit(f, grad, g, g_jac, lam, rho)
    # (the closed form of the same sum)
    np.testing.assert_allclose(M, f + ((np.maximum(lam + rho[:, None] * g, 0) ** 2 - lam ** 2).sum(axis=1)) / (2 * rho), rtol=1e-13)
    errs = {}
    for h in (1e-3, 1e-4, 1e-5, 1e-6, 1e-7):
        fd = np.zeros((K, n))
        for c in range(n):
            e = np.zeros(n)
            e[c] = h
            Mp = AR.merit(*_analytic(X + e), lam, rho)[0]
            Mm = AR.merit(*_analytic(X - e), lam, rho)[0]
            fd[:, c] = (Mp - Mm) / (2 * h)
        errs[h] = np.abs(fd - dM).max() / np.abs(dM).max()
    print("central differences of M against dM, relative to max |dM|:", {h: "%.1e" % e for h, e in errs.items()})
    assert errs[1e-5] <= 1e-9
    # an inactive row is not read: NaN there changes nothing; a NaN in g reaches M
    poisoned = np.where((psi == 0)[:, :, None], NAN, g_jac)
    M2, dM2 = AR.merit(f, grad, g, poisoned, lam, rho)
    assert np.array_equal(M2, M) and np.array_equal(dM2, dM)
    g_bad = g.copy()
    g_bad[1, 2] = NAN
    M3, _ = AR.merit(f, grad, g_bad, g_jac, lam, rho)
    assert np.isnan(M3[1]) and np.array_equal(np.delete(M3, 1), np.delete(M, 1))
    # longdouble in, longdouble out
    ld = lambda a: np.asarray(a, dtype=np.longdouble)         # noqa: E731
    Ml, dMl = AR.merit(ld(f), ld(grad), ld(g), ld(g_jac), ld(lam), ld(rho))
    assert Ml.dtype == dMl.dtype == np.longdouble
    np.testing.assert_allclose(np.asarray(Ml, dtype=np.float64), M, rtol=1e-14)


def test_convex_problem_reaches_its_kkt_point():
    """min 1/2 |x - a|^2, a = (1, 1, 0.2), subject to x_0 + x_1 <= 1 and x_2 <= 0.5 inside the box [-2, 2]: the projection of a onto the
    half-plane, x* = (0.5, 0.5, 0.2) with multipliers (0.5, 0).  Every start reaches both; the multiplier error contracts by
    1 / (1 + 2 rho) per outer iteration."""
    a = np.array([1.0, 1.0, 0.2])
    J = np.array([[1.0, 1.0, 0.0], [0.0, 0.0, 1.0]])

    def evaluate(X):
        d = X - a
        g = X @ J.T - np.array([1.0, 0.5])
        return 0.5 * (d * d).sum(axis=1), d, g, np.broadcast_to(J, (len(X), 2, 3)).copy()
    X0 = np.array([[0.0, 0.0, 0.0], [1.9, -1.5, 2.5], [-3.0, 1.0, 0.0]])
    trace = []
    x, info = AR.solve(evaluate, X0, -2.0, 2.0, outer_iterations=8, inner_ticks=25, trace=trace)
    print("x %s, lam %s, rho %s, violation %s, settled %s" % (info["x"], info["lam"], info["rho"], info["violation"], info["settled"]))
    # the iterates reach the KKT point; an incumbent is the cheapest point seen within feas_tol of the feasible set, so it may sit up to
    # feas_tol beyond the half-plane (and be that much cheaper)
    np.testing.assert_allclose(info["inner"]["X"], np.tile([0.5, 0.5, 0.2], (3, 1)), atol=1e-6)
    np.testing.assert_allclose(info["x"], np.tile([0.5, 0.5, 0.2], (3, 1)), atol=1e-4)
    assert np.all(info["x"][:, 0] + info["x"][:, 1] - 1.0 <= 1e-4) and np.all(info["f"] <= 0.25 + 1e-12)
    np.testing.assert_allclose(info["lam"], np.tile([0.5, 0.0], (3, 1)), atol=1e-5)
    np.testing.assert_allclose(info["f"], 0.25, atol=1e-4)
    assert info["feasible"].all() and info["settled"].all() and info["not_settled"] == 0 and info["alive"].all()
    assert info["evaluations"] <= 8 * 26 + 1 and info["best"] == int(np.lexsort((np.arange(3), info["f"], info["violation"]))[0])
    # incumbent keys never increase
    keys = [list(zip(t["state"]["inc_v"], t["state"]["inc_f"])) for t in trace]
    for before, after in zip(keys, keys[1:]):
        assert all(b2 <= b1 for b1, b2 in zip(before, after))


def test_outer_step_rule_and_finish():
    P = dict(growth=10.0, shrink=0.25, rho_max=50.0, lam_max=3.0, feas_tol=1e-4)
    st = AR.new_state(np.zeros((4, 2)), 2, rho0=10.0)
    X = np.arange(8.0).reshape(4, 2)
    f = np.array([1.0, 2.0, NAN, 3.0])
    g = np.array([[0.5, -1.0], [-1.0, 5e-5], [0.0, 0.0], [0.2, INF]])
    s1 = AR.outer(st, f, g, X, None, False, **P)
    assert s1["inc_v"].tolist() == [0.5, 0.0, INF, INF] and s1["inc_f"].tolist() == [1.0, 2.0, INF, INF]         # dead: 2 (f), 3 (g)
    assert np.array_equal(s1["inc_x"], [[0, 1], [2, 3], [0, 0], [0, 0]]) and not s1["lam"].any() and s1["V_prev"].tolist() == [INF] * 4
    s2 = AR.outer(s1, np.array([0.5, 2.5, 1.0, 1.0]), np.array([[0.6, 0.0], [-1.0, -1.0], [0.3, 0.4], [0.0, 0.0]]), X + 10, [1, 1, 0, 1], True, **P)
    assert s2["inc_v"].tolist() == [0.5, 0.0, 0.4, 0.0] and s2["inc_f"].tolist() == [1.0, 2.0, 1.0, 1.0]         # 0: cheaper but less feasible
    assert s2["lam"].tolist() == [[3.0, 0.0], [0.0, 0.0], [3.0, 3.0], [0.0, 0.0]]                               # clipped at lam_max and at 0
    assert s2["V_prev"].tolist() == [0.6, 0.0, 0.4, 0.0] and s2["rho"].tolist() == [10.0] * 4                   # V > 0.25 inf: never
    assert s2["settled"].tolist() == [False, True, False, True]
    s3 = AR.outer(s2, np.array([0.5, 2.5, 1.0, 1.0]), np.array([[0.1, 0.0], [-1.0, -1.0], [0.3, 0.4], [0.0, 0.0]]), X, [1] * 4, True, **P)
    assert s3["rho"].tolist() == [10.0, 10.0, 50.0, 10.0]                                                        # 0.1 <= 0.15; 0.4 > 0.1, capped
    assert s3["inc_v"][0] == 0.1 and np.array_equal(s3["inc_x"][0], X[0])
    assert AR.finish(s3, [1, 1, 1, 0]) == (3, (0.0, 1.0), 2)
    assert AR.finish({**s3, "inc_v": np.full(4, INF), "inc_f": np.full(4, INF)})[0] == 0


_c1 = {}


def _oracle_problem():
    """c1 = synth_problem(1, 100, 2, 2, 10, 64), trajectory 0, gamma = 1e-5, and the f = 0.3 row of
    tests/test_gpu_constraints.py::test_constrained_solve: one 95 % row on state 0, b = top - 0.3 span of mu_t0 + kappa sd_t0 along the
    unconstrained optimum from the zero start (here: lbfgs_reference on the oracle)."""
    if not _c1:
        import torch
        import lbfgs_reference as LR
        from constraints_reference import g_of_trajectory, reference_constraints
        from gaussian_process_mpc_amd.synth import synth_problem
        from oracle import cport, gpmpc_oracle as O
        pb = synth_problem(1, 100, 2, 2, 10, 64)
        gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"])
        H, da, x0 = pb["H"], pb["da"], pb["x0"][0]
        n = H * da

        def cost(X):                                         # (the C port of the oracle: the unconstrained solve only places the row)
            r = cport.rollout(pb, gp.Ky_inv.numpy(), 1e-5, x0=np.tile(x0, (len(X), 1)), U=X.reshape(-1, H, da))
            return r["cost"], r["grad"].reshape(len(X), n)
        U_free, free = LR.solve(cost, np.zeros((1, n)), -1.0, 1.0, max_ticks=150, history=8, gtol=1e-5, ftol=1e-12)
        A = np.array([[1.0, 0.0]])
        along = reference_constraints(gp, H, x0, U_free, A, [0.0], [K95], want_jac=False)["g"][:, 0]
        b = along.max() - 0.3 * (along.max() - along.min())
        T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))      # noqa: E731

        def one(u):                                          # cost, g and all their derivatives from ONE graph of the oracle's rollout
            Ut = T(u).clone().reshape(H, da).requires_grad_(True)
            means, covs = O.forward_propagate(gp, H, T(x0), Ut, "o2")
            c = O.cost(means, Ut, covs, T(pb["x_ref"]), T(pb["u_ref"]), pb["Q"], pb["R"], 1e-5)
            g = g_of_trajectory(means, [torch.diagonal(s) for s in covs], A, [b], [K95]).reshape(-1)
            out = torch.cat((c.reshape(1), g))
            (J,) = torch.autograd.grad(out, Ut, grad_outputs=torch.eye(len(out), dtype=torch.float64), is_grads_batched=True)
            return out.detach().numpy(), J.reshape(len(out), n).numpy()

        def evaluate(X):
            ev = [one(u) for u in X]
            return (np.array([o[0] for o, _ in ev]), np.array([J[0] for _, J in ev]), np.array([o[1:] for o, _ in ev]),
                    np.array([J[1:] for _, J in ev]))
        _c1.update(pb=pb, gp=gp, A=A, b=b, evaluate=evaluate, cost_free=float(free["f"][0]), U_free=U_free)
    return _c1


def test_rule_on_the_oracle_c1_zero_start():
    """The restatement on the pinned oracle, c1, zero start only (K = 1), the f = 0.3 row, 8 outer iterations x 25 ticks.  SLSQP on the
    same problem ends at 1.87492 (tests/test_gpu_constraints.py).  Observed: 209 evaluations of the oracle (about 0.2 s each: the
    8 x 25 is the default budget of the solver), cost 1.874919 at max g = 4.0e-5, rho = 1e5."""
    from constraints_reference import reference_constraints, reference_cost
    c = _oracle_problem()
    pb, gp = c["pb"], c["gp"]
    H, da, x0 = pb["H"], pb["da"], pb["x0"][0]
    print("unconstrained: cost %.6f (SLSQP construction: 1.86054), b = %.6f" % (c["cost_free"], c["b"]))
    np.testing.assert_allclose(c["cost_free"], 1.86054, rtol=1e-3)
    x, info = AR.solve(c["evaluate"], np.zeros((1, H * da)), -1.0, 1.0, outer_iterations=8, inner_ticks=25)
    viol = reference_constraints(gp, H, x0, x, c["A"], [c["b"]], [K95], want_jac=False)["g"].max()
    cost = reference_cost(gp, H, x0, x.reshape(H, da), pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], 1e-5)
    print("auglag on the oracle: %d evaluations, cost %.6f, max g %.3e, rho %s, settled %s, key %s" % (info["evaluations"], cost, viol, info["rho"], info["settled"],
                                                                                      (info["violation"][0], info["f"][0])))
    assert viol <= 1e-4
    np.testing.assert_allclose(cost, 1.87492, rtol=1e-3)
    assert np.all(np.abs(x) <= 1.0)


# ------------------------------------------------------------------------------------------------------------------------------
# the library: struct layout, state arithmetic, refusals without a device
# ------------------------------------------------------------------------------------------------------------------------------
def test_auglag_params_struct_layout_matches_header(built, tmp_path):
    from gaussian_process_mpc_amd._lib import AuglagParamsC, LbfgsParamsC
    names = [f[0] for f in AuglagParamsC._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpmpc.h"\nint main(){printf("%zu"' + ' " %zu"' * len(names)
                   + ', sizeof(gpmpc_auglag_params), ' + ", ".join("offsetof(gpmpc_auglag_params,%s)" % n for n in names) + ');return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(AuglagParamsC)
    assert out[1:] == [getattr(AuglagParamsC, n).offset for n in names]
    assert names == ["inner", "rho0", "growth", "shrink", "rho_max", "lam_max", "feas_tol", "inner_ticks", "reserved"]
    assert AuglagParamsC.rho0.offset == ctypes.sizeof(LbfgsParamsC)


def test_state_bytes_arithmetic_and_abi_surface(built):
    import re
    from gaussian_process_mpc_amd import _lib
    from gaussian_process_mpc_amd.device_auglag import SCALARS, auglag_state_layout
    lib = built.lib()
    r = lambda x: (x + 31) // 32 * 32                          # noqa: E731
    for K, H, da, mc in [(1, 1, 1, 1), (5, 10, 2, 3), (64, 65, 2, 16), (256, 20, 1, 2), (33, 7, 3, 5)]:
        n, R = H * da, H * mc
        by_hand = 32 + r(n) + 8 * r(K) + r(K * R) + r(K * n)                 # the table of include/gpmpc.h
        L = auglag_state_layout(K, n, R)
        assert lib.gpmpc_auglag_state_bytes(K, H, da, mc) == 8 * by_hand == 8 * L["total"]
        order = ["summary", "plan"] + list(SCALARS) + ["lam", "inc_x"]
        assert [L[f] for f in order] == sorted(L[f] for f in order) and L["summary"] == 0 and L["plan"] == 32
        assert all(L[f] % 32 == 0 for f in order) and (8 * L["total"]) % 256 == 0
    assert SCALARS == ("rho", "V_prev", "v", "f", "inc_v", "inc_f", "alive", "settled")
    for K, H, da, mc in [(0, 4, 2, 1), (257, 4, 2, 1), (4, 0, 2, 1), (4, 4, 0, 1), (4, 4, _lib.MAX_D + 1, 1), (4, 4, 2, 0), (4, 4, 2, 17)]:
        assert lib.gpmpc_auglag_state_bytes(K, H, da, mc) == 0
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpmpc.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gpmpc_[a-z_]+)\s*\(", hdr))
    for name in ("gpmpc_auglag_state_bytes", "gpmpc_auglag_merit", "gpmpc_auglag_outer", "gpmpc_auglag_solve",
                 "gpmpc_auglag_solve_workspace_bytes"):
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert declared == set(_lib.SIGNATURES)                  # the binding declares what the header declares


def test_auglag_entry_points_validate_arguments_without_a_device(built):
    from gaussian_process_mpc_amd import _lib
    from gaussian_process_mpc_amd._lib import CostParamsC, StateConstraintsC
    from gaussian_process_mpc_amd.device_auglag import auglag_params
    lib = built.lib()
    fake = ctypes.c_void_p(4096)                             # never dereferenced: every call below is refused before a launch
    big = 1 << 30
    good = lambda **kw: auglag_params(**{**dict(n_starts=4, da=2, lb=-1.0, ub=1.0), **kw})  # noqa: E731
    cost, cons = CostParamsC(), StateConstraintsC()
    cons.n_rows = 1
    ou = lambda P, H=4, da=2, mc=1, f=fake, g=fake, X=fake, s=fake, nb=big: lib.gpmpc_auglag_outer(   # noqa: E731
        H, da, mc, None if P is None else ctypes.byref(P), 1, f, g, X, None, None, s, nb, None)
    sv = lambda P, p=fake, H=4, x0=fake, X0=fake, c=cost, cs=cons, first=0, no=3, ws=fake: lib.gpmpc_auglag_solve(   # noqa: E731
        p, H, x0, X0, ctypes.byref(c) if c is not None else None, ctypes.byref(cs) if cs is not None else None,
        None if P is None else ctypes.byref(P), first, no, ws, big, None)
    me = lambda K=4, H=4, da=2, mc=1, a=(fake,) * 8: lib.gpmpc_auglag_merit(K, H, da, mc, *a, None)   # noqa: E731
    assert me(K=0) == -1 and me(H=0) == -1 and me(da=0) == -1 and me(da=_lib.MAX_D + 1) == -1 and me(mc=0) == -1 and me(mc=_lib.MAX_CONS + 1) == -1
    for i in range(8):
        assert me(a=tuple(None if j == i else fake for j in range(8))) == -1
    assert ou(None) == -1 and ou(good(), f=None) == -1 and ou(good(), g=None) == -1 and ou(good(), X=None) == -1 and ou(good(), s=None) == -1
    assert ou(good(), H=0) == -1 and ou(good(), mc=0) == -1 and ou(good(), mc=17) == -1 and ou(good(), da=9) == -1
    assert ou(good(), nb=lib.gpmpc_auglag_state_bytes(4, 4, 2, 1) - 8) == -4               # GPMPC_E_WORKSPACE
    for call in (ou, sv):
        for name in ("rho0", "growth", "rho_max"):
            for bad in (0.0, -1.0, NAN):
                assert call(good(**{name: bad})) == -1 and (name + " =").encode() in lib.gpmpc_last_error(), (name, bad)
        assert call(good(growth=0.5)) == -1 and b"growth" in lib.gpmpc_last_error()
        for bad in (0.0, -0.1, 1.5, NAN):
            assert call(good(shrink=bad)) == -1 and b"shrink" in lib.gpmpc_last_error(), bad
        for name in ("feas_tol", "lam_max"):
            for bad in (-1e-300, NAN):
                assert call(good(**{name: bad})) == -1 and name.encode() in lib.gpmpc_last_error(), (name, bad)
        for bad in (0, -3):
            assert call(good(inner_ticks=bad)) == -1 and b"inner_ticks" in lib.gpmpc_last_error()
        # what the embedded L-BFGS parameters refuse
        for K in (0, _lib.LBFGS_MAX_STARTS + 1):
            assert call(good(n_starts=K)) == -1 and b"n_starts" in lib.gpmpc_last_error()
        assert call(good(history=17)) == -1 and b"history" in lib.gpmpc_last_error()
        for name in ("gtol", "ftol", "c1", "min_step"):
            assert call(good(**{name: NAN})) == -1 and name.encode() in lib.gpmpc_last_error()
    assert sv(good(), no=-1) == -1 and b"n_outer" in lib.gpmpc_last_error()
    assert sv(good(), first=-1) == -1 and b"first_outer" in lib.gpmpc_last_error()
    assert sv(good(), p=None) == -1 and sv(None) == -1 and sv(good(), H=0) == -1 and sv(good(), c=None) == -1 and sv(good(), cs=None) == -1
    assert sv(good(), x0=None) == -1 and sv(good(), ws=None) == -1 and sv(good(), X0=None) == -1
    bad_rows, bad_kappa = StateConstraintsC(), StateConstraintsC()
    bad_rows.n_rows, bad_kappa.n_rows = 17, 2
    bad_kappa.kappa[1] = -1.0
    assert sv(good(), cs=bad_rows) == -1 and b"n_rows" in lib.gpmpc_last_error()
    assert sv(good(), cs=bad_kappa) == -1 and b"kappa[1]" in lib.gpmpc_last_error()
    wb = lib.gpmpc_auglag_solve_workspace_bytes
    assert wb(None, 4, ctypes.byref(cons), ctypes.byref(good())) == 0 and wb(fake, 4, None, ctypes.byref(good())) == 0
    assert wb(fake, 4, ctypes.byref(cons), None) == 0 and wb(fake, 4, ctypes.byref(bad_rows), ctypes.byref(good())) == 0
    assert wb(fake, 4, ctypes.byref(cons), ctypes.byref(good(n_starts=0))) == 0
    assert wb(fake, 4, ctypes.byref(cons), ctypes.byref(good(history=17))) == 0


def test_solver_argument_needs_no_device():
    import torch
    from gaussian_process_mpc_amd.mpc import RiskSensitiveMPC
    mpc = RiskSensitiveMPC.__new__(RiskSensitiveMPC)
    mpc.horizon, mpc.state_dim, mpc.input_dim = 5, 2, 1
    mpc.full_covariance, mpc.train_empty, mpc.n_starts, mpc.solver, mpc.state_constraints = False, False, 1, None, None
    mpc.device = torch.device("cpu")
    with pytest.raises(ValueError, match="None, 'mppi', 'lbfgs' or 'auglag'"):          # the message lists all four
        mpc.get_optimal_trajectory(np.zeros(2), solver="cma")
    with pytest.raises(ValueError, match="without state constraints.*lbfgs"):
        mpc.get_optimal_trajectory(np.zeros(2), solver="auglag")
    mpc.solver = "auglag"                                    # the attribute is read like the argument
    with pytest.raises(ValueError, match="lbfgs"):
        mpc.get_optimal_trajectory(np.zeros(2), n_starts=4)
    mpc.state_constraints, mpc.full_covariance = object(), True
    with pytest.raises(NotImplementedError, match="full-covariance"):
        mpc.get_optimal_trajectory(np.zeros(2))
    # what refused before still refuses: lbfgs with constraints, a host multi-start with constraints
    mpc.full_covariance = False
    with pytest.raises(NotImplementedError, match="state constraints"):
        mpc.get_optimal_trajectory(np.zeros(2), solver="lbfgs")
    # the options of a fresh object are the defaults of auglag_solve
    import inspect
    from gaussian_process_mpc_amd.device_auglag import auglag_solve
    sig = inspect.signature(auglag_solve).parameters
    src = inspect.getsource(RiskSensitiveMPC.__init__)
    assert "auglag_options" in src
    for name in ("outer", "inner_ticks", "rho0", "growth", "shrink", "rho_max", "lam_max", "feas_tol", "history", "gtol", "ftol", "check_outer"):
        assert name in sig and ('"%s": ' % name) in src, name
    assert (sig["outer"].default, sig["inner_ticks"].default, sig["rho0"].default, sig["feas_tol"].default) == (8, 25, 10.0, 1e-4)
