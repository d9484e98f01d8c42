"""Holds tests/particle_cost_reference.py itself and everything of the particle-cost entry points that needs no device (CPU):

  * the C ABI: names, argument counts against the header, every refusal before any launch, workspace sizes;
  * the statistical pin of the rule: on Gaussian particles (numpy draws, P = 4096, ds = 3, fixed seeds) the stage cost sits within 4
    delta-method standard errors of the closed form the cost kernels evaluate (cost_reference.state_terms) at gamma in {0, 1e-3, 1, -0.3},
    and the quantile of a row within 4 standard errors of a . mu + kappa sd - b;
  * the controls: gamma with the wrong sign, the mean in the place of the entropic risk, the order statistic one place off -- each misses
    by a wide, printed factor;
  * the table of m_r = floor(eps_r P + 1e-9)."""
import ctypes
import math
import os
import re
from statistics import NormalDist

import numpy as np
import pytest

import cost_reference as CR
import particle_cost_reference as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gpmpc_particle_cost", "gpmpc_particle_evaluate_workspace_bytes", "gpmpc_particle_evaluate",
         "gpmpc_mppi_solve_particles_workspace_bytes", "gpmpc_mppi_solve_particles"]
E_ARG, E_WORKSPACE = -1, -4


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_mpc_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_abi_names_and_signatures(L):
    from gaussian_process_mpc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    assert re.search(r"#define\s+GPMPC_PARTICLE_COST_MAX_P\s+4096\b", hdr) and _lib.PARTICLE_COST_MAX_P == 4096
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        res, args = _lib.SIGNATURES[name]
        assert res in (ctypes.c_int, ctypes.c_size_t)
        assert getattr(L, name) is not None
        n_decl = len(re.search(r"\b%s\s*\((.*?)\);" % name, hdr, flags=re.S).group(1).split(","))
        assert n_decl == len(args), (name, n_decl, len(args))
    import gaussian_process_mpc_amd as g
    for name in ("particle_cost", "particle_evaluate", "mppi_solve_particles"):
        assert hasattr(g, name) and name in g.__all__
    assert g.RiskSensitiveMPC.particle_options == {"particles": 256}


def test_not_provided_lists_no_longer_name_the_planner():
    for f in ("include/gpmpc.h", "README.md", "DESIGN.md"):
        assert "a particle-cost MPPI" not in open(os.path.join(ROOT, f)).read(), f


def _cost_c(ds=2, da=1, gamma=0.5, schedule_id=0):
    from gaussian_process_mpc_amd._lib import CostParamsC
    c = CostParamsC()
    c.gamma = gamma
    for k in range(ds):
        c.Q[k * ds + k] = 1.0
    for k in range(da):
        c.R[k * da + k] = 1.0
    c.schedule_id = schedule_id
    return c


def test_refusals_before_any_launch(L):
    """Every refusal is decided on the host: GPMPC_E_ARG with a text that names the entry (no device is touched: this runs without one)."""
    from gaussian_process_mpc_amd._lib import StateConstraintsC, MppiParamsC
    from test_host_particles import MODEL_REFUSALS, _model_c
    p = ctypes.c_void_p(4096)
    big = 1 << 40
    ok, cost = _model_c(), _cost_c()
    cons, bad_rows, nan_kappa = StateConstraintsC(), StateConstraintsC(), StateConstraintsC()
    cons.n_rows, bad_rows.n_rows, nan_kappa.n_rows = 1, 17, 1
    nan_kappa.kappa[0] = float("nan")
    ref = lambda c: None if c is None else ctypes.byref(c)  # noqa: E731

    def pcost(B=2, P=3, H=2, ds=2, da=1, cost=cost, cons=None, part=p, U=p, out=p, stage=None, g=None):
        return L.gpmpc_particle_cost(B, P, H, ds, da, ref(cost), ref(cons), part, U, out, stage, g, None)

    def peval(m=ok, B=2, P=3, H=2, x0=p, U=p, cost=cost, cons=None, out=p, stage=None, g=None, chunk=64, ws=p, nb=big):
        return L.gpmpc_particle_evaluate(ref(m), B, P, H, x0, U, 1, 0, ref(cost), ref(cons), out, stage, g, chunk, ws, nb, None)

    def params(K=8, iters=2, sigma=1.0, decay=0.9, beta=0.1, lb=-1.0, ub=1.0):
        P = MppiParamsC()
        P.n_samples, P.iterations, P.sigma_decay, P.beta, P.seed = K, iters, decay, beta, 1
        P.sigma[0], P.lb[0], P.ub[0] = sigma, lb, ub
        return P

    def solve(m=ok, H=2, P=3, x0=p, start=p, cost=cost, cons=None, prm=None, U=p, best=p, trace=p, ws=p, nb=big):
        prm = params() if prm is None else prm
        return L.gpmpc_mppi_solve_particles(ref(m), H, P, x0, start, ref(cost), ref(cons), ctypes.byref(prm), U, best, trace, ws, nb, None)

    def refused(rc, text, who):
        msg = L.gpmpc_last_error().decode()
        assert rc == E_ARG and text in msg and who in msg, (rc, text, msg)

    for text, kw in MODEL_REFUSALS.items():                   # everything gpmpc_particle_rollout refuses of a model
        bad = _model_c(**kw)
        refused(peval(m=bad), text, "gpmpc_particle_evaluate")
        refused(solve(m=bad), text, "gpmpc_mppi_solve_particles")
    shared = {"B < 1": dict(B=0), "P < 1": dict(P=0), "GPMPC_PARTICLE_COST_MAX_P": dict(P=4097), "H outside": dict(H=0), "NULL pointer (cost)": dict(cost=None),
              "cost schedule": dict(cost=_cost_c(schedule_id=12345)), "n_rows": dict(cons=bad_rows, g=p), "kappa": dict(cons=nan_kappa, g=p),
              "exactly when": dict(cons=cons), "exactly": dict(g=p), "NULL pointer": dict(out=None), "NULL": dict(U=None), "2^31": dict(B=70000, P=4096), "B > 65535": dict(B=65536, P=3)}
    for text, kw in shared.items():
        refused(pcost(**kw), text, "gpmpc_particle_cost")
        refused(peval(**kw), text, "gpmpc_particle_evaluate")
    for text, kw in {"state_dim": dict(ds=0), "state_dim = 9": dict(ds=9, da=0), "action_dim": dict(ds=8, da=1), "NULL pointer": dict(part=None)}.items():
        refused(pcost(**kw), text, "gpmpc_particle_cost")
    for text, kw in {"chunk": dict(chunk=96), "chunk must": dict(chunk=-64), "NULL pointer": dict(x0=None), "NULL": dict(ws=None)}.items():
        refused(peval(**kw), text, "gpmpc_particle_evaluate")
    assert peval(nb=L.gpmpc_particle_evaluate_workspace_bytes(ctypes.byref(ok), 2, 3, 2, 64) - 1) == E_WORKSPACE
    for text, kw in {"n_samples": dict(prm=params(K=0)), "n_samples = 4097": dict(prm=params(K=4097)), "iterations": dict(prm=params(iters=0)),
                     "sigma_decay": dict(prm=params(decay=0.0)), "beta": dict(prm=params(beta=-1.0)), "sigma[0]": dict(prm=params(sigma=0.0)),
                     "lb[0]": dict(prm=params(lb=2.0)), "H < 1": dict(H=0), "NULL pointer": dict(x0=None), "NULL": dict(trace=None),
                     "P < 1": dict(P=0), "GPMPC_PARTICLE_COST_MAX_P": dict(P=5000), "cost schedule": dict(cost=_cost_c(schedule_id=777)),
                     "n_rows": dict(cons=bad_rows), "kappa": dict(cons=nan_kappa), "what a solver takes": dict(m=_model_c(ds=2, da=0))}.items():
        refused(solve(**kw), text, "gpmpc_mppi_solve_particles")
    prm = params()
    assert solve(nb=L.gpmpc_mppi_solve_particles_workspace_bytes(ctypes.byref(ok), 2, 3, ctypes.byref(prm), None) - 1) == E_WORKSPACE


def test_workspace_sizes(L):
    from gaussian_process_mpc_amd._lib import StateConstraintsC, MppiParamsC
    from test_host_particles import _model_c
    m = ctypes.byref(_model_c(n=70, ds=2, da=1))
    ev, step, roll = L.gpmpc_particle_evaluate_workspace_bytes, L.gpmpc_particle_step_workspace_bytes, L.gpmpc_particle_rollout_workspace_bytes
    # two particle buffers, the noise, the stage costs and one step: monotone in B, P and H, and NO term proportional to H B P
    assert ev(m, 2, 70, 3, 64) >= step(m, 2, 70, 64) + 8 * (2 * 140 * 2 + 70 * 3 + 2 * 4)
    assert ev(m, 2, 70, 3, 64) <= ev(m, 4, 70, 3, 64) and ev(m, 2, 70, 3, 64) <= ev(m, 2, 140, 3, 64) and ev(m, 2, 70, 3, 64) <= ev(m, 2, 70, 30, 64)
    assert ev(m, 2, 70, 4000, 64) - ev(m, 2, 70, 3, 64) <= 8 * 2 * 4000 + 512              # only the stage costs grow with H
    assert roll(m, 2, 70, 4000, 64) - roll(m, 2, 70, 3, 64) >= 8 * 3996 * 140 * 2            # (to a 256-byte section boundary;the stored rollout does grow with H B P)
    for bad in ((0, 70, 3, 64), (2, 0, 3, 64), (2, 4097, 3, 64), (2, 70, 0, 64), (2, 70, 3, 100), (2, 70, 3, -64)):
        assert ev(m, *bad) == 0, bad
    prm = MppiParamsC()
    prm.n_samples = 16
    cons = StateConstraintsC()
    cons.n_rows = 2
    sv = L.gpmpc_mppi_solve_particles_workspace_bytes
    free, held = sv(m, 3, 70, ctypes.byref(prm), None), sv(m, 3, 70, ctypes.byref(prm), ctypes.byref(cons))
    assert free >= ev(m, 16, 70, 3, 0) + 8 * (16 * 3 + 16 * 2 + 16 + 3 + 2 * 5) and held >= free + 8 * 16 * 3 * 2
    assert sv(m, 3, 0, ctypes.byref(prm), None) == 0 and sv(m, 3, 4097, ctypes.byref(prm), None) == 0 and sv(m, 0, 70, ctypes.byref(prm), None) == 0
    cons.n_rows = 17
    assert sv(m, 3, 70, ctypes.byref(prm), ctypes.byref(cons)) == 0
    prm.n_samples = 0
    assert sv(m, 3, 70, ctypes.byref(prm), None) == 0


# ------------------------------------------------------------------------------------------------------------------ the rule
P_PIN, DS_PIN = 4096, 3
GAMMAS = (0.0, 1e-3, 1.0, -0.3)


def _gaussian_particles(seed):
    """mu, Sigma, a symmetric positive definite Q, x_ref and P_PIN numpy draws of N(mu, Sigma).  Sigma and Q are small enough that
    I + 2 gamma Q Sigma is positive definite for every gamma of the grid: exp(-(gamma / 2) c) then has a variance and the delta method
    applies."""
    rng = np.random.default_rng(seed)
    Bm = rng.standard_normal((DS_PIN, DS_PIN))
    Sigma = 0.08 * Bm @ Bm.T / DS_PIN + 0.02 * np.eye(DS_PIN)
    Am = rng.standard_normal((DS_PIN, DS_PIN))
    Q = 0.5 * Am @ Am.T / DS_PIN + 0.4 * np.eye(DS_PIN)
    mu, xref = rng.uniform(-0.6, 0.6, DS_PIN), rng.uniform(-0.3, 0.3, DS_PIN)
    X = mu + rng.standard_normal((P_PIN, DS_PIN)) @ np.linalg.cholesky(Sigma).T
    for g in GAMMAS:
        assert np.linalg.eigvalsh(np.eye(DS_PIN) + 2.0 * g * np.linalg.cholesky(Sigma).T @ Q @ np.linalg.cholesky(Sigma)).min() > 0.2
    return dict(mu=mu, Sigma=Sigma, Q=Q, xref=xref, X=X)


def _closed_form(pb, gamma):
    return float(CR.state_terms(pb["Q"], pb["Sigma"][None], (pb["mu"] - pb["xref"])[None], gamma)["value"][0])


def _stage_z(pb, gamma, **wrong):
    """(estimate - closed form) / delta-method standard error: se = sd(c) / sqrt P at gamma = 0, else (2 / |gamma|) sd(w) / (mean(w) sqrt P)
    with w = exp(-(gamma / 2) c)."""
    s = PC.stage(pb["X"], pb["Q"], pb["xref"], gamma, **wrong)
    c = s["c"].astype(np.float64)
    if gamma == 0.0:
        se = c.std(ddof=1) / math.sqrt(P_PIN)
    else:
        w = np.exp(-(gamma / 2.0) * c)
        se = (2.0 / abs(gamma)) * w.std(ddof=1) / (w.mean() * math.sqrt(P_PIN))
    return (float(s["value"]) - _closed_form(pb, gamma)) / se


@pytest.mark.parametrize("seed", [3, 5])
def test_stage_cost_is_the_closed_form_within_four_standard_errors(seed):
    pb = _gaussian_particles(seed)
    for gamma in GAMMAS:
        z = _stage_z(pb, gamma)
        print("  seed %d gamma %+.0e: closed form %.6f, z = %+.2f" % (seed, gamma, _closed_form(pb, gamma), z))
        assert abs(z) <= 4.0
    # controls at gamma = 1, each to miss by twice the band (|z| > 8 has probability below 1e-15 under the rule): the wrong sign of gamma, and the mean in the place of the entropic risk
    z = _stage_z(pb, 1.0, gamma_sign=-1.0)
    print("  seed %d control gamma = 1 with the wrong sign: z = %+.1f" % (seed, z))
    assert abs(z) > 8.0
    z = _stage_z(pb, 1.0, mean_only=True)
    print("  seed %d control mean in the place of the entropic risk at gamma = 1: z = %+.1f" % (seed, z))
    assert abs(z) > 8.0


@pytest.mark.parametrize("seed", [3, 5])
def test_quantile_is_the_gaussian_rule_within_four_standard_errors(seed):
    pb = _gaussian_particles(seed)
    rng = np.random.default_rng([seed, 1])
    nd = NormalDist()
    for prob in (0.5, 0.9, 0.95, 0.99):
        a, b = rng.standard_normal(DS_PIN), 0.3
        kappa = nd.inv_cdf(prob)
        sd = math.sqrt(a @ pb["Sigma"] @ a)
        want = a @ pb["mu"] + kappa * sd - b
        se = math.sqrt(prob * (1.0 - prob) / P_PIN) * sd / nd.pdf(kappa)
        z = (float(PC.rows(pb["X"], a, b, kappa)["g"][0]) - want) / se
        print("  seed %d prob %.2f: m = %d, z = %+.2f" % (seed, prob, PC.quantile_counts(kappa, P_PIN)[0], z))
        assert abs(z) <= 4.0
    # control: one place off is already outside the rounding budget of the GPU test by a wide factor (an order statistic, not a smooth
    # function: neighbours differ by about se / sqrt(p (1 - p) P), some 1e-4 of the unit, against a budget of 1e-12 of it)
    a, kappa = rng.standard_normal(DS_PIN), nd.inv_cdf(0.95)
    r0 = PC.rows(pb["X"], a, 0.3, kappa)
    for shift in (-1, 1):
        miss = abs(float(PC.rows(pb["X"], a, 0.3, kappa, index_shift=shift)["g"][0] - r0["g"][0])) / (1e-12 * float(r0["unit"][0]))
        print("  seed %d control index P - m %+d: misses by %.3g budgets" % (seed, shift, miss))
        assert miss > 1e3


def test_quantile_counts_table():
    """m_r for p in {.5, .9, .95, .99} x P in {1, 20, 100, 256, 300, 4096} is floor((1 - p) P) in exact arithmetic: the 1e-9 guard absorbs
    the rounding of erfc where (1 - p) P is an integer."""
    nd = NormalDist()
    for prob, den in ((0.5, 2), (0.9, 10), (0.95, 20), (0.99, 100)):
        for P in (1, 20, 100, 256, 300, 4096):
            assert PC.quantile_counts(nd.inv_cdf(prob), P)[0] == P // den, (prob, P)
    assert PC.quantile_counts(0.0, 7)[0] == 3 and PC.quantile_counts([0.0, 40.0], 4096).tolist() == [2048, 0]


def test_reference_nan_and_composition():
    """A NaN coordinate makes exactly its (plan, step) NaN; the cost is the sum of the stages and the input terms of cost_reference."""
    rng = np.random.default_rng(5)
    X = rng.standard_normal((4, 3, 9, 2))
    U = rng.standard_normal((3, 3, 1))
    kw = dict(gamma=0.7, Q=np.array([[1.0, 0.2], [0.0, 0.5]]), R=np.array([[0.3]]), Rd=np.array([[0.1]]), last_u=np.array([0.2]))
    cons = (np.array([[1.0, 0.0], [0.3, -0.8]]), np.array([0.1, -0.2]), np.array([0.0, 1.0]))
    r = PC.cost(X, U, cons=cons, **kw)
    assert np.allclose((r["cost"] - r["stage"].sum(axis=1) - CR.input_terms(U, kw["R"], kw["Rd"], kw["last_u"])["value"]).astype(float), 0.0, atol=1e-15)
    Xn = X.copy()
    Xn[2, 1, 4, 0] = np.nan
    rn = PC.cost(Xn, U, cons=cons, **kw)
    nan_stage, nan_g = np.isnan(rn["stage"].astype(float)), np.isnan(rn["g"].astype(float))
    want_stage, want_g = np.zeros((3, 4), bool), np.zeros((3, 3, 2), bool)
    want_stage[1, 2], want_g[1, 1, :] = True, True
    assert np.array_equal(nan_stage, want_stage) and np.array_equal(nan_g, want_g) and np.isnan(rn["cost"].astype(float)).tolist() == [False, True, False]
    keep = ~want_stage
    assert np.array_equal(rn["stage"][keep], r["stage"][keep]) and np.array_equal(rn["g"][~want_g], r["g"][~want_g])
