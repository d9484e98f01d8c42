"""Holds tests/feedback_inputs_reference.py itself and everything of the commanded input under feedback that needs no device (CPU):

  * the reference's input-constraint Jacobian and the gradient its cost seed gives through the adjoint sweep equal torch autograd of a
    float64 restatement of the values through the chain of steps (tests/test_host_linprop_fc.py's ``value_f64``, step after step), within
    the budget the GPU tests use (1e-12 sum |terms| plus 4 ulp of the value; the packed Jacobians of the chain enter with their own
    bound E as |J| + E / tol, which covers their error to first order and beyond);
  * each deliberate mistake of the reference misses that budget by at least 100 on inputs chosen for it: a general R, a row that is not
    axis-aligned, gains that differ from step to step;
  * a closed form at ds = da = 1;
  * the C ABI: names, argument types, exports, and every refusal of the header as GPMPC_E_ARG before any launch (check_refusals is also
    called by tests/test_gpu_feedback_inputs.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import feedback_inputs_reference as I
import linprop_fc_reference as F
import linprop_reference as R
import test_host_linprop_fc as HF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gpmpc_feedback_input_cost", "gpmpc_feedback_input_constraints", "gpmpc_linearised_fc_rollout_inputs_workspace_bytes",
         "gpmpc_linearised_fc_rollout_inputs", "gpmpc_particle_inputs", "gpmpc_particle_step_inputs_workspace_bytes", "gpmpc_particle_step_inputs",
         "gpmpc_particle_input_stats", "gpmpc_particle_rollout_feedback_workspace_bytes", "gpmpc_particle_rollout_feedback"]
E_ARG, E_WORKSPACE = -1, -4
TOL, ULP, f64 = 1e-12, 2.0 ** -52, R.G.to_f64


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_mpc_amd import _lib
    return _lib.lib()


def problem(case="nonsym_nominal_noise", B=2, H=3, seed=7):
    """A model, plans, per-step gains that differ, a general (non-symmetric) R and three rows: one not axis-aligned, one with kappa = 0."""
    m = HF.CASES[case]()
    ds, da, _ = R.dims(m)
    rng = np.random.default_rng(seed)
    x0, U = rng.uniform(-1.0, 1.0, (B, ds)), rng.uniform(-1.0, 1.0, (B, H, da))
    K = rng.uniform(-0.5, 0.5, (H, da, ds))
    Rm = rng.uniform(0.2, 1.0, (da, da)) + np.eye(da)
    C = np.concatenate([np.eye(da)[:1], -np.eye(da)[-1:], rng.uniform(0.3, 1.0, (1, da)) * np.where(np.arange(da) % 2, -1.0, 1.0)])
    d, kappa = np.array([1.5, 1.2, 0.8]), np.array([1.6, 0.0, 2.0])
    return m, x0, U, K, Rm, C, d, kappa


def chain_units(ch):
    """|J| + E / tol of the chain's packed Jacobians, E the bound the steps are held to."""
    E = np.stack([TOL * f64(s["jac_abs"]) + 4 * ULP * f64(s["jac_mag"]) for s in ch["steps"]], axis=1)
    return np.abs(f64(ch["jac"])) + E / TOL


# ------------------------------------------------------------------------------------------------------------------ the reference itself
def torch_values(m, x0, U, K, Rm, C, d, kappa):
    """(c, g_u (H m), covs (H+1, ds, ds)) of ONE plan in float64 torch from U (H, da): the chain of HF.value_f64 steps on the packed state."""
    ds, da, _ = R.dims(m)
    P0 = np.asarray(R.noise_model(m)[0], dtype=np.float64)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    pairs = F.tri_pairs(ds)
    s = t(F.pack_state(np.asarray(x0, dtype=np.float64), P0))
    c, g, covs = 0.0, [], []
    for k in range(U.shape[0] + 1):
        rows = [[None] * ds for _ in range(ds)]
        for i, (a, b) in enumerate(pairs):
            rows[a][b] = rows[b][a] = s[ds + i]
        S = torch.stack([torch.stack(r) for r in rows])
        covs.append(S.detach().numpy())
        if k == U.shape[0]:
            break
        Kt = t(K[k])
        Su = Kt @ S @ Kt.T
        c = c + (t(Rm) * Su).sum()                                           # tr(R Su^T) = sum_ab R_ab Su_ab (Su symmetric)
        q = torch.einsum("rj,jk,rk->r", t(C), Su, t(C))
        g.append(t(C) @ U[k] + t(kappa) * torch.sqrt(q) - t(d))
        s = HF.value_f64(m, torch.cat([s, U[k]]), K[k])
    return c, torch.cat(g), np.stack(covs)


@pytest.mark.parametrize("case", list(HF.CASES))
def test_reference_jacobian_and_seed_are_autograd_of_the_value(case):
    m, x0, U, K, Rm, C, d, kappa = problem(case)
    kappa = np.array([1.6, 0.5, 2.0])                                        # (autograd of sqrt is the variance part everywhere)
    ds, da, _ = R.dims(m)
    B, H = U.shape[0], U.shape[1]
    ch = F.chain(m, x0, U, K)
    units = chain_units(ch)
    ic = I.input_constraints(U, ch["covs"], ch["jac"], K, C, d, kappa, jac_units=units)
    co = I.input_cost(ch["covs"], K, Rm)
    grad = F.sweep(ch["jac"], None, co["dcovs"])[0]
    A_grad = F.sweep(units, None, co["A_dcovs"])[0]
    worst = [0.0] * 4
    for b in range(B):
        Ub = torch.as_tensor(U[b])
        c, g, cv = torch_values(m, x0[b], Ub, K, Rm, C, d, kappa)
        vc, vg = I.input_cost(cv[None], K, Rm), I.input_constraints(U[b:b + 1], cv[None], None, K, C, d, kappa)    # the values on ITS covariances
        gc = torch.autograd.functional.jacobian(lambda y: torch_values(m, x0[b], y, K, Rm, C, d, kappa)[0], Ub).numpy()
        gj = torch.autograd.functional.jacobian(lambda y: torch_values(m, x0[b], y, K, Rm, C, d, kappa)[1], Ub).numpy().reshape(H * 3, H * da)
        bj = TOL * f64(ic["A_gjac"][b]) + 4 * ULP * np.abs(f64(ic["gjac"][b]))
        exact = f64(ic["A_gjac"][b]) == 0                                    # tau >= t: zeros and the direct part
        assert np.array_equal(gj[exact], f64(ic["gjac"][b])[exact])
        worst[0] = max(worst[0], float((np.abs(c.item() - f64(vc["c"][0])) / (TOL * f64(vc["A_c"][0]))).max()))
        worst[1] = max(worst[1], float((np.abs(g.numpy().reshape(H, 3) - f64(vg["g"][0])) / (TOL * f64(vg["A_g"][0]))).max()))
        bg = TOL * f64(A_grad[b]) + 4 * ULP * np.abs(f64(grad[b]))
        assert np.array_equal(gc[bg == 0], f64(grad[b])[bg == 0]) and not np.any(gc[H - 1])      # the last input moves no Sigma_j, j < H
        worst[2] = max(worst[2], float((np.abs(gc - f64(grad[b]))[bg > 0] / bg[bg > 0]).max()))
        worst[3] = max(worst[3], float((np.abs(gj - f64(ic["gjac"][b]))[~exact] / bj[~exact]).max()))
    print("  %s: c %.3g, g_u %.3g, gradient of c %.3g, Jacobian of g_u %.3g of the budget against autograd" % ((case,) + tuple(worst)))
    assert max(worst) <= 1.0
    # row t = 0 has only its tau = 0 block
    assert np.array_equal(f64(ic["gjac"])[:, :3, :da], np.broadcast_to(C, (B, 3, da))) and not np.any(f64(ic["gjac"])[:, :3, da:])


MISTAKES = ["offdiag_once", "gain_of_next_step", "cov_after_step", "R_transposed"]


def mistake_factor(name):
    """By how many budgets the reference with mistake ``name`` misses the reference: the worst entry of c, the seed, g_u and its Jacobian."""
    m, x0, U, K, Rm, C, d, kappa = problem()
    ch = F.chain(m, x0, U, K)
    covs, jac = f64(ch["covs"]), f64(ch["jac"])
    ic, co = I.input_constraints(U, covs, jac, K, C, d, kappa), I.input_cost(covs, K, Rm)
    kc = {k: True for k in (name,) if k in ("gain_of_next_step", "cov_after_step", "R_transposed")}
    kg = {k: True for k in (name,) if k != "R_transposed"}
    bc, bg = I.input_cost(covs, K, Rm, **kc), I.input_constraints(U, covs, jac, K, C, d, kappa, **kg)
    fs = []
    for good, bad, key, unit in ((co, bc, "c", "A_c"), (co, bc, "dcovs", "A_dcovs"), (ic, bg, "g", "A_g"), (ic, bg, "gjac", "A_gjac")):
        b = TOL * f64(good[unit]) + 4 * ULP * np.abs(f64(good[key]))
        fs.append(float((np.abs(f64(bad[key] - good[key])) / np.where(b > 0, b, np.inf)).max()))
    return fs


@pytest.mark.parametrize("name", MISTAKES)
def test_each_mistake_misses_the_budget(name):
    fs = mistake_factor(name)
    print("  mistake %s: misses by %.3g (c), %.3g (seed), %.3g (g_u), %.3g (Jacobian) budgets" % ((name,) + tuple(fs)))
    assert max(fs) >= 100.0
    if name == "offdiag_once":
        assert fs[3] >= 100.0 and fs[0] == fs[1] == fs[2] == 0.0
    elif name == "R_transposed":
        assert fs[1] >= 100.0 and fs[0] == 0.0
    elif name == "cov_after_step":                                           # (the seed does not read the covariances)
        assert min(fs[0], fs[2], fs[3]) >= 100.0 and fs[1] == 0.0
    else:
        assert min(fs) >= 100.0


def test_closed_form_scalar():
    """ds = da = 1: c = R K^2 sum_{t<H} Sigma_t, sd = |K c| sqrt(Sigma_t)."""
    rng = np.random.default_rng(0)
    H, Kg, Rr, cc, dd, kap = 4, -0.7, 1.3, -2.0, 0.4, 1.5
    S, U = rng.uniform(0.01, 0.1, (2, H + 1, 1, 1)), rng.uniform(-1, 1, (2, H, 1))
    co = I.input_cost(S, [[Kg]], [[Rr]])
    assert np.abs(f64(co["c"]) - Rr * Kg * Kg * S[:, :H, 0, 0].sum(1)).max() <= 1e-15
    assert np.abs(f64(co["dcovs"])[:, :H, 0, 0] - Rr * Kg * Kg).max() <= 1e-15 and not np.any(f64(co["dcovs"])[:, H])
    ic = I.input_constraints(U, S, None, [[Kg]], [[cc]], [dd], [kap])
    assert np.abs(f64(ic["sd"])[:, :, 0] - abs(Kg * cc) * np.sqrt(S[:, :H, 0, 0])).max() <= 1e-15
    assert np.abs(f64(ic["g"])[:, :, 0] - (cc * U[:, :, 0] + kap * abs(Kg * cc) * np.sqrt(S[:, :H, 0, 0]) - dd)).max() <= 1e-15
    u, _ = I.particle_inputs(rng.standard_normal((2, 5, 1)), U[:, 0], [[Kg]], np.zeros((2, 1)))
    assert u.shape == (2, 5, 1)


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_abi_names_signatures_and_exports(L):
    from gaussian_process_mpc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    assert "the commanded input" in hdr and "w_kk = a_k^2" in hdr and "tr(R K_j Sigma_j K_j^T)" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"typedef struct gpmpc_input_constraints \{[^}]*\bC\[GPMPC_MAX_CONS \* GPMPC_MAX_D\][^}]*\bd\[GPMPC_MAX_CONS\]", hdr)
    for name in NAMES:
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_size_t if name.endswith("_bytes") else ctypes.c_int)
        assert getattr(L, name) is not None
        decl = re.search(r"\b%s\s*\((.*?)\);" % name, hdr, flags=re.S).group(1).split(",")
        assert len(decl) == len(args), (name, len(decl), len(args))
        for text, ty in zip(decl, args):                                     # pointers are pointers, sizes are size_t, ints are ints
            # (c_size_t and c_ulonglong are one ctypes type where both are 64 bits)
            scalars = {ctypes.c_int: ("int",), ctypes.c_uint: ("unsigned",), ctypes.c_size_t: ("size_t", "unsigned long long")}
            want = "*" in text if ty not in scalars else (any(w in text for w in scalars[ty]) and "*" not in text)
            assert want, (name, text)
    assert ctypes.sizeof(_lib.InputConstraintsC) == 8 + 8 * (_lib.MAX_CONS * _lib.MAX_D + 2 * _lib.MAX_CONS)
    import gaussian_process_mpc_amd as g
    for name in ("InputConstraints", "feedback_input_cost", "feedback_input_constraints", "particle_inputs", "particle_step_inputs",
                 "particle_input_stats"):
        assert hasattr(g, name) and name in g.__all__
    import inspect
    for fn in (g.linearised_rollout, g.mppi_solve_linearised):
        pr = inspect.signature(fn).parameters
        assert pr["input_cost"].default is False and pr["input_constraints"].default is None
    pr = inspect.signature(g.particle_rollout).parameters
    assert pr["feedback"].default is None and pr["mean_ref"].default is None and pr["input_constraints"].default is None
    assert inspect.signature(g.RiskSensitiveMPC.validate_plan).parameters["feedback"].default is False
    for name in ("set_input_constraints", "set_input_chance_bounds", "clear_input_constraints"):
        assert hasattr(g.RiskSensitiveMPC, name)
    assert g.RiskSensitiveMPC.feedback_input_cost is False
    ic = g.InputConstraints.box([-1.0, None], [2.0, 3.0], 2, prob=0.95)
    assert ic.m == 3 and ic.da == 2 and ic.c.n_rows == 3 and list(ic.c.C[:6]) == [1.0, 0.0, 0.0, 1.0, -1.0, 0.0] and list(ic.c.d[:3]) == [2.0, 3.0, 1.0]
    assert abs(ic.kappa[0] - 1.6448536269514722) < 1e-12
    with pytest.raises(ValueError):
        g.InputConstraints([[1.0]], [1.0])


def check_refusals(L):
    """Every refusal the header lists for the new entries: GPMPC_E_ARG with a text, and 0 from the size query.  The pointers are not device
    memory: a call that got as far as a launch would fault or return GPMPC_E_LAUNCH, not GPMPC_E_ARG."""
    from gaussian_process_mpc_amd._lib import CostParamsC, InputConstraintsC, StateConstraintsC
    p = ctypes.c_void_p
    a, b, c_, d, e = (p(0x2000 + 0x100 * i) for i in range(5))
    kk, ws, big = p(0x8000), p(0x9000), 1 << 40
    count = 0

    def refused(rc, what, who="gpmpc_"):
        nonlocal count
        assert rc == E_ARG, (what, rc)
        assert L.gpmpc_last_error().decode().startswith(who), (what, L.gpmpc_last_error())
        count += 1

    cost = CostParamsC()
    cost.Q[0] = cost.Q[3] = cost.R[0] = 1.0
    uc = InputConstraintsC()
    uc.n_rows, uc.C[0], uc.d[0], uc.kappa[0] = 1, 1.0, 1.0, 1.0
    bad_rows, bad_kappa, nan_kappa = InputConstraintsC(), InputConstraintsC(), InputConstraintsC()
    bad_rows.n_rows = 17
    bad_kappa.n_rows, bad_kappa.kappa[0] = 1, -1.0
    nan_kappa.n_rows, nan_kappa.kappa[0] = 1, float("nan")
    zero_rows = InputConstraintsC()

    def fcost(B=1, H=3, ds=2, da=1, cp=cost, K=kk, ks=0, covs=a, oc=b, od=c_):
        return L.gpmpc_feedback_input_cost(B, H, ds, da, None if cp is None else ctypes.byref(cp), K, ks, covs, oc, od, None)

    for kw in (dict(cp=None), dict(covs=None), dict(oc=None), dict(B=0), dict(H=0), dict(ds=0), dict(ds=9), dict(da=0), dict(ds=5, da=4),
               dict(ks=1), dict(ks=3), dict(H=64 * 65535 + 1)):
        refused(fcost(**kw), "input cost %s" % kw, "gpmpc_feedback_input_cost")

    def fcons(B=1, H=3, ds=2, da=1, C=uc, K=kk, ks=0, U=a, covs=b, jac=c_, g=d, gj=e):
        return L.gpmpc_feedback_input_constraints(B, H, ds, da, None if C is None else ctypes.byref(C), K, ks, U, covs, jac, g, gj, None)

    for kw in (dict(C=None), dict(U=None), dict(covs=None), dict(g=None), dict(jac=None), dict(B=0), dict(H=0), dict(ds=9), dict(da=0),
               dict(ds=5, da=4), dict(C=bad_rows), dict(C=zero_rows), dict(C=bad_kappa), dict(C=nan_kappa), dict(ks=1), dict(ks=3),
               dict(H=64 * 65535 + 1)):
        refused(fcons(**kw), "input constraints %s" % kw, "gpmpc_feedback_input_constraints")

    who = "gpmpc_linearised_fc_rollout_inputs"

    def roll(m, B=4, H=3, x0=a, U=b, K=None, ks=0, cp=None, cons=None, flags=0, jac=None, oc=None, og=None, g=None, gj=None, icost=0, ucons=None,
             gu=None, guj=None, chunk=0, w=ws):
        return L.gpmpc_linearised_fc_rollout_inputs(ctypes.byref(m), B, H, x0, U, K, ks, None if cp is None else ctypes.byref(cp),
                                                    None if cons is None else ctypes.byref(cons), flags, None, None, jac, oc, og, g, gj, icost,
                                                    None if ucons is None else ctypes.byref(ucons), gu, guj, chunk, w, big, None)

    good, noact = HF._model_c(), HF._model_c(da=0)
    # what the sibling entry refuses
    for field, value in (("state_dim", 0), ("state_dim", 9), ("action_dim", -1), ("n", 0), ("ld", 5), ("X", None)):
        m = HF._model_c()
        setattr(m, field, value)
        refused(roll(m), "rollout " + field, who)
    m = HF._model_c()
    m.has_noise, m.init_cov[0], m.init_cov[3], m.init_cov[1], m.init_cov[2] = 1, 1e-3, 1e-3, 5e-4, 4e-4
    refused(roll(m), "asymmetric init_cov", who)
    cons = StateConstraintsC()
    cons.n_rows, cons.A[0], cons.kappa[0] = 1, 1.0, 1.0
    for kw in (dict(B=0), dict(H=0), dict(chunk=32), dict(flags=4), dict(flags=2), dict(x0=None), dict(U=None), dict(w=None), dict(K=kk, ks=1),
               dict(ks=5), dict(jac=c_), dict(cp=cost), dict(cp=cost, oc=c_, flags=1), dict(cons=cons), dict(cons=cons, g=c_, flags=1),
               dict(B=1, H=64 * 65535 + 1)):
        refused(roll(good, **kw), "rollout %s" % kw, who)
    refused(roll(noact, U=None, K=kk), "a gain with da = 0", who)
    # the new arguments
    refused(roll(good, icost=1), "input_cost without a cost", who)
    refused(roll(noact, U=None, ucons=uc, gu=d), "input constraints with da = 0", who)
    refused(roll(good, ucons=uc), "ucons without out_gu", who)
    refused(roll(good, ucons=uc, gu=d, flags=1), "ucons + grad without out_gujac", who)
    refused(roll(good, ucons=uc, gu=d, guj=e), "out_gujac without WANT_GRAD", who)
    refused(roll(good, gu=d), "out_gu without ucons", who)
    refused(roll(good, guj=e, flags=1), "out_gujac without ucons", who)
    for bad in (bad_rows, zero_rows, bad_kappa, nan_kappa):
        refused(roll(good, ucons=bad, gu=d), "bad rows", who)
    refused(roll(good, K=kk, ks=3, ucons=uc, gu=d), "k_step_stride 3", who)
    rz = L.gpmpc_linearised_fc_rollout_inputs_workspace_bytes
    old = L.gpmpc_linearised_fc_rollout_workspace_bytes
    gm = ctypes.byref(good)
    assert rz(gm, 4, 3, 4, 0, 0, None) == 0 and rz(gm, 4, 0, 0, 0, 0, None) == 0 and rz(gm, 4, 3, 0, 100, 0, None) == 0
    assert rz(ctypes.byref(noact), 4, 3, 0, 0, 1, None) == 0 and rz(ctypes.byref(noact), 4, 3, 0, 0, 0, ctypes.byref(uc)) == 0
    assert rz(gm, 4, 3, 0, 0, 0, ctypes.byref(bad_rows)) == 0
    assert rz(gm, 4, 3, 1, 0, 1, ctypes.byref(uc)) == old(gm, 4, 3, 1, 0) > rz(gm, 4, 3, 0, 0, 0, None) == old(gm, 4, 3, 0, 0) > 0
    assert L.gpmpc_linearised_fc_rollout_inputs(gm, 4, 3, a, b, None, 0, None, None, 0, None, None, None, None, None, None, None, 0, None, None,
                                                None, 0, ws, 16, None) == E_WORKSPACE
    # the particles under feedback
    who = "gpmpc_particle"

    def fpi(B=1, P=4, ds=2, da=1, x=a, U=b, us=1, K=kk, mu=c_, ms=2, out=d):
        return L.gpmpc_particle_inputs(B, P, ds, da, x, U, us, K, mu, ms, out, None)

    for kw in (dict(B=0), dict(P=0), dict(ds=0), dict(ds=9), dict(da=0), dict(da=8), dict(ds=5, da=4), dict(x=None), dict(U=None), dict(out=None),
               dict(mu=None), dict(B=2, us=0), dict(B=2, ms=1)):
        refused(fpi(**kw), "particle inputs %s" % kw, who)

    def fst(B=1, P=4, H=3, da=1, inp=a, C=uc, um=b, ucv=c_, uv=d, uj=e):
        return L.gpmpc_particle_input_stats(B, P, H, da, inp, None if C is None else ctypes.byref(C), um, ucv, uv, uj, None)

    for kw in (dict(B=0), dict(P=0), dict(H=0), dict(H=65536), dict(B=65536), dict(da=0), dict(da=8), dict(inp=None), dict(C=bad_rows),
               dict(C=bad_kappa), dict(C=None), dict(uv=None), dict(uj=None)):
        refused(fst(**kw), "input stats %s" % kw, who)

    def fsi(m=good, B=2, P=4, x=a, Up=b, eps=c_, nxt=d, chunk=0, w=ws):
        return L.gpmpc_particle_step_inputs(ctypes.byref(m), B, P, x, Up, eps, nxt, None, None, chunk, w, big, None)

    for kw in (dict(m=noact), dict(B=0), dict(P=0), dict(chunk=32), dict(x=None), dict(Up=None), dict(eps=None), dict(nxt=None), dict(w=None)):
        refused(fsi(**kw), "step with inputs %s" % kw, who)
    sz = L.gpmpc_particle_step_inputs_workspace_bytes
    assert sz(ctypes.byref(noact), 2, 4, 0) == 0 and sz(gm, 0, 4, 0) == 0 and sz(gm, 2, 4, 0) == L.gpmpc_particle_step_workspace_bytes(gm, 2, 4, 0) > 0
    assert L.gpmpc_particle_step_inputs(gm, 2, 4, a, b, c_, d, None, None, 0, ws, 16, None) == E_WORKSPACE
    o1, o2, o3 = p(0x3000), p(0x3100), p(0x3200)

    def frf(m=good, B=2, P=4, H=3, x0=a, U=b, part=c_, mean=d, cov=e, cl=o1, K=None, ks=0, mu=None, C=None, um=o2, ucv=o3, uv=None, uj=None,
            chunk=0, w=ws, wb=big):
        return L.gpmpc_particle_rollout_feedback(ctypes.byref(m), B, P, H, x0, U, 5, 0, None, part, mean, cov, cl, None, None, K, ks, mu,
                                                 None if C is None else ctypes.byref(C), None, um, ucv, uv, uj, chunk, w, wb, None)

    bad_model = HF._model_c()
    bad_model.n = 0
    for kw in (dict(m=noact, U=None), dict(m=bad_model), dict(B=0), dict(P=0), dict(H=0), dict(chunk=32), dict(x0=None), dict(U=None), dict(part=None),
               dict(um=None), dict(ucv=None), dict(w=None), dict(K=kk), dict(ks=1), dict(ks=3), dict(C=bad_rows, uv=a, uj=b),
               dict(C=nan_kappa, uv=a, uj=b), dict(C=uc), dict(C=uc, uv=a), dict(uv=a), dict(uj=b)):
        refused(frf(**kw), "rollout under feedback %s" % kw, who)
    rf = L.gpmpc_particle_rollout_feedback_workspace_bytes
    assert rf(ctypes.byref(noact), 2, 4, 3, 0, 1) == 0 and rf(gm, 2, 4, 0, 0, 1) == 0 and rf(gm, 2, 4, 3, 32, 1) == 0
    assert rf(gm, 2, 4, 3, 0, 0) > rf(gm, 2, 4, 3, 0, 1) == L.gpmpc_particle_rollout_workspace_bytes(gm, 2, 4, 3, 0) > 0
    assert frf(wb=16) == E_WORKSPACE
    return count


def test_every_refusal_comes_before_a_launch(L):
    n = check_refusals(L)
    print("  %d refusals, each GPMPC_E_ARG with a text" % n)
    assert n >= 110
