"""Holds tests/linprop_reference.py itself and everything of the linearised propagation that needs no device (CPU):

  * the reference's analytic step Jacobian equals torch.autograd.functional.jacobian of its own float64 value function, within the
    term-sum budget the GPU tests use (1e-12 sum |terms|, carried through the composite outputs, plus 4 ulp of the sizes the last float64
    additions round at);
  * with v = 0 and action_var = 0 the step IS the pointwise posterior of tests/particle_reference.py;
  * each deliberate mistake of the reference (r = 2 K k, the h term dropped, the nominal weights left out of g) misses that budget by at
    least 100 on the test inputs: the budget discriminates;
  * the C ABI: names, signatures, exports, and every refusal of the header, which comes back as GPMPC_E_ARG without a device -- before any
    launch (check_refusals is also called by tests/test_gpu_linprop.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import linprop_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gpmpc_linearised_step_workspace_bytes", "gpmpc_linearised_step", "gpmpc_linearised_rollout_workspace_bytes",
         "gpmpc_linearised_rollout", "gpmpc_mppi_solve_linearised_workspace_bytes", "gpmpc_mppi_solve_linearised"]
E_ARG, E_WORKSPACE = -1, -4
TOL = 1e-12
ULP = 2.0 ** -52
f64 = R.G.to_f64


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_mpc_amd import _lib
    return _lib.lib()


def bound(ref, key):
    """tol * budget + 4 ulp of the magnitudes, float64."""
    return TOL * f64(ref[key + "_abs"]) + 4.0 * ULP * f64(ref[key + "_mag"])


# ------------------------------------------------------------------------------------------------------------------ the reference itself
def value_f64(model, x):
    """(mu', var') of ONE column from x = (mu, var, u) in float64 torch: g is written out, its derivative (the h term) is autograd's."""
    ds, da, D = R.dims(model)
    _, av, pv = R.noise_model(model)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    mu, var, u = x[:ds], x[ds:2 * ds], x[2 * ds:]
    z, S = torch.cat([mu, u]), torch.cat([var, t(av)])
    X, beta = t(model["X"]), t(model["beta"])
    out_m, out_v = [], []
    for a in range(ds):
        lam, sf = t(model["lam"][a]), float(model["sf"][a])
        diff = X - z[None, :]
        k = sf * sf * torch.exp(-0.5 * (diff * diff / lam[None, :]).sum(1))
        bk = beta[:, a] * k
        m = bk.sum()
        g = (bk[:, None] * diff / lam[None, :]).sum(0)
        if model.get("nominal") is not None:
            W, b = t(model["nominal"][0])[a], float(np.broadcast_to(model["nominal"][1], (ds,))[a])
            m = m + W @ z + b
            g = g + W
        K = t(R.P._kinv(model, a))
        q = k @ (K @ k)
        out_m.append(m)
        out_v.append((sf * sf - q) + (g * g * S).sum() + float(pv[a]))
    return torch.stack(out_m + out_v)


@pytest.mark.parametrize("case", ["pergp", "nonsym_nominal_noise", "shared"])
def test_reference_jacobian_is_autograd_of_its_value(case):
    m = {"pergp": lambda: R.make_model(40, 2, 1),
         "nonsym_nominal_noise": lambda: R.make_model(33, 3, 2, "nonsym", noise=True, nominal=True, pair=True),
         "shared": lambda: R.make_model(20, 2, 2, "shared")}[case]()
    mu, var, U = R.make_inputs(m, 3)
    ref = R.step(m, mu, var, U)
    worst = 0.0
    for c in range(3):
        x = torch.as_tensor(np.concatenate([mu[c], var[c], U[c]]))
        val = value_f64(m, x).numpy()
        J = torch.autograd.functional.jacobian(lambda y: value_f64(m, y), x).numpy()
        ds = mu.shape[1]
        assert np.all(np.abs(val[:ds] - f64(ref["mu"][c])) <= TOL * f64(ref["m_abs"][c]))
        assert np.all(np.abs(val[ds:] - f64(ref["var"][c])) <= bound(ref, "var")[c])
        ratio = np.abs(J - f64(ref["jac"][c])) / np.where(bound(ref, "jac")[c] > 0, bound(ref, "jac")[c], 1.0)
        assert np.all((bound(ref, "jac")[c] > 0) | (J == 0))                 # the structural zeros (d mu' / d var) are zeros of both
        worst = max(worst, float(ratio.max()))
    print("  %s: analytic Jacobian vs autograd, worst %.3g of the budget" % (case, worst))
    assert worst <= 1.0


def test_zero_input_variance_is_the_pointwise_posterior():
    m = R.make_model(50, 2, 1, nominal=True)
    m.update(init_cov=np.zeros((2, 2)), action_var=np.zeros(1), process_var=np.array([2e-3, 0.0]))
    mu, _, U = R.make_inputs(m, 5)
    ref = R.step(m, mu, np.zeros_like(mu), U)
    post = R.P.posterior(m, np.concatenate([mu, U], axis=1))
    em = np.abs(f64(ref["mu"] - post["m"])) / (TOL * f64(post["m_abs"]))
    ev = np.abs(f64(ref["var"] - post["s2"])) / (TOL * f64(post["q_abs"]))
    print("  v = 0: mean %.3g, variance %.3g of the budget" % (em.max(), ev.max()))
    assert em.max() <= 1.0 and ev.max() <= 1.0


CONTROLS = [("r_twice", dict(kind="nonsym")), ("drop_h", dict(kind="pergp")), ("drop_nominal_g", dict(kind="pergp", nominal=True))]


def control_factor(m, mu, var, U, name):
    """By how many budgets the reference with mistake `name` misses the reference: the worst entry of var' and the Jacobian."""
    ref, bad = R.step(m, mu, var, U), R.step(m, mu, var, U, **{name: True})
    fj = np.abs(f64(bad["jac"] - ref["jac"])) / np.where(bound(ref, "jac") > 0, bound(ref, "jac"), np.inf)
    fv = np.abs(f64(bad["var"] - ref["var"])) / bound(ref, "var")
    return max(float(fj.max()), float(fv.max()))


@pytest.mark.parametrize("name,kw", CONTROLS, ids=[c[0] for c in CONTROLS])
def test_each_control_misses_the_budget(name, kw):
    m = R.make_model(70, 2, 1, **kw)
    mu, var, U = R.make_inputs(m, 3)
    factor = control_factor(m, mu, var, U, name)
    print("  control %s: misses by %.3g budgets" % (name, factor))
    assert factor >= 100.0


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_abi_names_signatures_and_exports(L):
    from gaussian_process_mpc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    assert "Linearised propagation" in hdr and "h_ad" in hdr and "(Kinv_a + Kinv_a^T) k" in hdr      # the rule is in the comment
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        res, args = _lib.SIGNATURES[name]
        assert res in (ctypes.c_int, ctypes.c_size_t)
        assert getattr(L, name) is not None
        n_decl = len(re.search(r"\b%s\s*\((.*?)\);" % name, hdr, flags=re.S).group(1).split(","))
        assert n_decl == len(args), (name, n_decl, len(args))
    import gaussian_process_mpc_amd as g
    for name in ("linearised_step", "linearised_rollout", "mppi_solve_linearised"):
        assert hasattr(g, name) and name in g.__all__
    from gaussian_process_mpc_amd import linearised
    assert linearised.linearised_rollout is g.linearised_rollout
    assert hasattr(g.RiskSensitiveMPC, "propagation")


def _model_c(n=10, ds=2, da=1):
    from gaussian_process_mpc_amd._lib import GPModelC
    c = GPModelC()
    c.n, c.state_dim, c.action_dim = n, ds, da
    c.X = c.beta = c.Kinv = 0x1000                       # never dereferenced: every call below is refused before a launch
    c.ld, c.gp_stride = n, 0
    for k in range(ds * (ds + da)):
        c.lambdas[k] = 1.5
    for a in range(ds):
        c.sigma_f[a] = 1.0
    return c


def check_refusals(L):
    """Every refusal the header lists for the three entries: GPMPC_E_ARG with a text, and 0 from the size queries.  The pointers are not
    device memory: a call that got as far as a launch would fault or return GPMPC_E_LAUNCH, not GPMPC_E_ARG."""
    from gaussian_process_mpc_amd._lib import CostParamsC, MppiParamsC, StateConstraintsC
    p = ctypes.c_void_p
    a, b, c_, d, e = (p(0x2000 + 0x100 * i) for i in range(5))
    ws, big = p(0x9000), 1 << 40
    count = 0

    def refused(rc, what):
        nonlocal count
        assert rc == E_ARG, (what, rc)
        assert L.gpmpc_last_error().decode().startswith("gpmpc_"), what
        count += 1

    def step(m, B=4, mu=a, var=b, U=c_, us=1, om=d, ov=e, jac=None, js=0, chunk=0, w=ws):
        return L.gpmpc_linearised_step(ctypes.byref(m), B, mu, var, U, us, om, ov, jac, js, chunk, w, big, None)

    def roll(m, B=4, H=3, x0=a, U=b, cost=None, cons=None, flags=0, means=None, vars_=None, jac=None, oc=None, og=None, g=None, gj=None,
             chunk=0, w=ws):
        return L.gpmpc_linearised_rollout(ctypes.byref(m), B, H, x0, U, None if cost is None else ctypes.byref(cost),
                                          None if cons is None else ctypes.byref(cons), flags, means, vars_, jac, oc, og, g, gj, chunk, w, big, None)

    good = _model_c()
    # the model
    for field, value in (("state_dim", 0), ("state_dim", 9), ("action_dim", -1), ("action_dim", 7), ("n", 0), ("ld", 5), ("X", None),
                         ("beta", None), ("Kinv", None)):
        m = _model_c()
        setattr(m, field, value)
        refused(step(m), "step " + field)
        refused(roll(m), "rollout " + field)
    for arr, k, value in (("lambdas", 1, 0.0), ("lambdas", 2, float("inf")), ("sigma_f", 1, -1.0), ("sigma_f", 0, float("nan"))):
        m = _model_c()
        getattr(m, arr)[k] = value
        refused(step(m), "step " + arr)
    m = _model_c()
    m.has_nominal, m.nom_w[1] = 1, float("nan")
    refused(step(m), "nominal")
    for arr, k, value in (("init_cov", 3, -1e-3), ("init_cov", 0, float("nan")), ("action_var", 0, -1.0), ("process_var", 1, float("inf"))):
        m = _model_c()
        m.has_noise = 1
        getattr(m, arr)[k] = value
        refused(step(m), "step " + arr)
        refused(roll(m), "rollout " + arr)
    # the step
    refused(step(good, B=0), "B")
    refused(step(good, chunk=-64), "chunk < 0")
    refused(step(good, chunk=100), "chunk % 64")
    for kw in (dict(mu=None), dict(var=None), dict(U=None), dict(om=None), dict(ov=None), dict(w=None)):
        refused(step(good, **kw), "step NULL %s" % kw)
    refused(step(good, om=a), "aliasing")
    refused(step(good, us=0), "u_stride")
    refused(step(good, jac=p(0x7000), js=5), "jac_stride")
    assert L.gpmpc_linearised_step_workspace_bytes(ctypes.byref(good), 0, 1, 0) == 0
    assert L.gpmpc_linearised_step_workspace_bytes(ctypes.byref(good), 4, 1, 100) == 0
    assert L.gpmpc_linearised_step_workspace_bytes(ctypes.byref(good), 4, 1, 0) > L.gpmpc_linearised_step_workspace_bytes(ctypes.byref(good), 4, 0, 0) > 0
    assert L.gpmpc_linearised_step(ctypes.byref(good), 4, a, b, c_, 1, d, e, None, 0, 0, ws, 16, None) == E_WORKSPACE
    # the rollout
    cost = CostParamsC()
    cost.Q[0] = cost.Q[3] = cost.R[0] = 1.0
    cons = StateConstraintsC()
    cons.n_rows, cons.A[0], cons.kappa[0] = 1, 1.0, 1.0
    refused(roll(good, B=0), "B")
    refused(roll(good, H=0), "H")
    refused(roll(good, chunk=32), "chunk")
    for flags in (4, 8, 16, 5, 2):
        refused(roll(good, flags=flags), "flags %d" % flags)
    refused(roll(good, x0=None), "x0")
    refused(roll(good, U=None), "U")
    refused(roll(good, w=None), "workspace")
    refused(roll(good, jac=c_), "out_jac without WANT_GRAD")
    refused(roll(good, cost=cost), "cost without out_cost")
    refused(roll(good, cost=cost, oc=c_, flags=1), "cost + grad without out_grad")
    refused(roll(good, cons=cons), "cons without out_g")
    refused(roll(good, cons=cons, g=c_, flags=1), "cons + grad without out_gjac")
    bad_cons = StateConstraintsC()
    bad_cons.n_rows = 17
    refused(roll(good, cons=bad_cons, g=c_), "n_rows")
    bad_cons.n_rows, bad_cons.kappa[0] = 1, -1.0
    refused(roll(good, cons=bad_cons, g=c_), "kappa")
    sched = CostParamsC()
    sched.schedule_id = 987654
    rc = roll(good, cost=sched, oc=c_)
    assert rc == E_ARG and "cost schedule" in L.gpmpc_last_error().decode()
    refused(roll(good, cost=cost, oc=c_, H=3000), "H beyond the cost kernel")
    noact = _model_c(da=0)
    refused(roll(noact, U=None, cost=cost, oc=c_), "cost with da = 0")
    assert L.gpmpc_linearised_rollout_workspace_bytes(ctypes.byref(good), 4, 3, 4, 0) == 0
    assert L.gpmpc_linearised_rollout_workspace_bytes(ctypes.byref(good), 4, 0, 0, 0) == 0
    assert L.gpmpc_linearised_rollout_workspace_bytes(ctypes.byref(good), 4, 3, 1, 0) > L.gpmpc_linearised_rollout_workspace_bytes(ctypes.byref(good), 4, 3, 0, 0) > 0
    assert L.gpmpc_linearised_rollout(ctypes.byref(good), 4, 3, a, b, None, None, 0, None, None, None, None, None, None, None, 0, ws, 16, None) == E_WORKSPACE
    # the MPPI solve
    P = MppiParamsC()
    P.n_samples, P.iterations, P.sigma_decay, P.beta = 8, 2, 0.9, 0.1
    P.sigma[0], P.lb[0], P.ub[0] = 0.5, -1.0, 1.0

    def solve(m=good, H=3, x0=a, start=b, cst=cost, cn=None, par=P, oU=c_, ob=d, ot=e, w=ws):
        return L.gpmpc_mppi_solve_linearised(ctypes.byref(m), H, x0, start, None if cst is None else ctypes.byref(cst),
                                             None if cn is None else ctypes.byref(cn), None if par is None else ctypes.byref(par), oU, ob, ot, w, big, None)

    for kw in (dict(x0=None), dict(start=None), dict(cst=None), dict(par=None), dict(oU=None), dict(ob=None), dict(ot=None), dict(w=None), dict(H=0)):
        refused(solve(**kw), "solve %s" % kw)
    for field, value in (("n_samples", 0), ("n_samples", 4097), ("iterations", 0), ("sigma_decay", 0.0), ("beta", float("nan"))):
        Q = MppiParamsC.from_buffer_copy(P)
        setattr(Q, field, value)
        refused(solve(par=Q), "solve " + field)
    Q = MppiParamsC.from_buffer_copy(P)
    Q.sigma[0] = 0.0
    refused(solve(par=Q), "sigma")
    Q = MppiParamsC.from_buffer_copy(P)
    Q.lb[0] = 2.0
    refused(solve(par=Q), "lb > ub")
    refused(solve(cn=bad_cons), "solve kappa")
    refused(solve(m=noact), "solve da = 0")
    m = _model_c()
    m.sigma_f[0] = 0.0
    refused(solve(m=m), "solve model")
    assert solve(cst=sched) == E_ARG
    assert L.gpmpc_mppi_solve_linearised_workspace_bytes(ctypes.byref(good), 3, ctypes.byref(P), None) > 0
    assert L.gpmpc_mppi_solve_linearised_workspace_bytes(ctypes.byref(noact), 3, ctypes.byref(P), None) == 0
    assert L.gpmpc_mppi_solve_linearised(ctypes.byref(good), 3, a, b, ctypes.byref(cost), None, ctypes.byref(P), c_, d, e, ws, 16, None) == E_WORKSPACE
    return count


def test_every_refusal_comes_before_a_launch(L):
    n = check_refusals(L)
    print("  %d refusals, each GPMPC_E_ARG with a text" % n)
    assert n >= 75
