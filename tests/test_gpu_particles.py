"""GPU tests of the particle entry points against tests/particle_reference.py (long double; include/gpmpc.h, "Particles").

Shapes are the smallest at which the tiling can go wrong: n in {1, 63, 70, 130} (ragged 16-deep stages and 64-row edges, two and three
row blocks), nq in {1, 65, 200} with chunk = 64 (200 spans four chunks) and the default chunk, D up to its maximum.

Bounds.  m: 1e-12 sum |beta_i k_i|.  q: 1e-12 sum |k_i K_ij k_j| -- the budget tests/test_gpu_gpstate.py holds gpmpc_predict's dot products
to.  The library returns s2 = (sf^2 - q) + process_var, not q: the two float64 roundings of that line are allowed on top, 2 ulp of
sf^2 + process_var (1 ulp = 2^-52 of the value), and nothing else."""
import functools

import numpy as np
import pytest
import torch

import particle_reference as R

pytestmark = pytest.mark.gpu
TOL = 1e-12
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    return g


def f64(a):
    return R.G.to_f64(a)


def same_bits(a, b):
    """torch.equal on the bit patterns (the covariance of ONE particle is NaN, and must be the same NaN)."""
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


# ------------------------------------------------------------------------------------------------------------------ models
@functools.lru_cache(maxsize=None)
def model_data(n, ds, da, kind="pergp", seed=0, sn=0.1, process_var=False, nominal=False):
    """A GP bundle on random inputs.  kind: pergp (per-GP hyper-parameters and inverses; with ds = 4 the GPs 0, 2 and 1, 3 share theirs: two
    groups of two) | shared (one hyper-parameter set, ONE inverse, gp_stride = 0) | ld (shared, row stride n + 5) | nonsym (per-GP,
    every entry of the inverse perturbed by a relative 1e-3: not symmetric, which pins the sum over ALL entries)."""
    rng = np.random.default_rng(100 * n + 10 * ds + da + seed)
    D = ds + da
    X = rng.uniform(-1.5, 1.5, (n, D))
    lam = rng.uniform(1.0, 3.0, (ds, D))
    sf = rng.uniform(0.6, 1.8, ds)
    if kind in ("shared", "ld"):
        lam, sf = np.tile(lam[:1], (ds, 1)), np.tile(sf[:1], ds)
    elif ds == 4:
        lam[2], sf[2], lam[3], sf[3] = lam[0], sf[0], lam[1], sf[1]
    Y = np.stack([np.sin(X @ rng.standard_normal(D)) for _ in range(ds)], axis=1) + sn * rng.standard_normal((n, ds))
    Ks = []
    for a in range(ds):
        K = f64(R.G.kernel(X, X, lam[a], sf[a])) + sn * sn * np.eye(n)
        Ki = np.linalg.inv(K)                                             # LU (getrf / getri): not symmetric to the last bit
        if kind == "nonsym":
            Ki = Ki * (1.0 + 1e-3 * rng.standard_normal((n, n)))
        Ks.append(Ki)
    Kinv = Ks[0] if kind in ("shared", "ld") else np.stack(Ks)
    beta = np.stack([Ks[a] @ Y[:, a] for a in range(ds)], axis=1)
    m = dict(X=X, beta=beta, Kinv=Kinv, lam=lam, sf=sf, kind=kind)
    if process_var:
        m.update(init_cov=np.diag(np.full(ds, 2e-3)), action_var=np.full(da, 1e-3), process_var=rng.uniform(1e-3, 4e-3, ds))
    if nominal:
        m["nominal"] = (0.1 * rng.standard_normal((ds, D)), 0.05 * rng.standard_normal(ds))
    return m


def device_model(G, m):
    ds, da, _ = R.dims(m)
    K = m["Kinv"]
    if m.get("kind") == "ld":
        n = K.shape[0]
        buf = torch.full((n, n + 5), float("nan"), dtype=torch.float64, device="cuda")
        buf[:, :n] = torch.as_tensor(K)
        K = buf[:, :n]
    gm = G.GPModel(m["X"], m["beta"], K, m["lam"], m["sf"], ds, da, nominal=m.get("nominal"), init_cov=m.get("init_cov"),
                   action_var=m.get("action_var"), process_var=m.get("process_var"))
    if m.get("kind") == "ld":
        assert gm.c.ld == K.shape[0] + 5 and gm.c.gp_stride == 0
    return gm


def queries(m, nq, seed=3):
    ds, da, D = R.dims(m)
    return np.random.default_rng(seed).uniform(-1.2, 1.2, (nq, D))


def var_tol(m, ref):
    pv = R.noise_model(m)[2]
    return TOL * f64(ref["q_abs"]) + 2.0 * ULP * (np.asarray(m["sf"]) ** 2 + pv)[None, :]


def worst_posterior(m, ref, mean, var, rows=slice(None)):
    em = np.abs(mean - f64(ref["m"][rows])) / (TOL * f64(ref["m_abs"][rows]))
    ev = np.abs(var - f64(ref["s2"][rows])) / var_tol(m, ref)[rows]
    return float(em.max()), float(ev.max())


# ------------------------------------------------------------------------------------------------------------------ gp_posterior
@pytest.mark.parametrize("dims", [(1, 1), (2, 1), (4, 1), (8, 0)], ids=lambda d: "ds%d_da%d" % d)
@pytest.mark.parametrize("n", [1, 63, 70, 130])
def test_gp_posterior_grid(G, n, dims):
    ds, da = dims
    kind = ("pergp", "shared", "ld", "pergp")[(n + ds) % 4]               # every kind meets ragged and multi-block sizes
    m = model_data(n, ds, da, kind, process_var=(n % 2 == 0), nominal=(ds == 2))
    gm = device_model(G, m)
    Z = queries(m, 200)
    ref = R.posterior(m, Z)
    for nq in (1, 65, 200):
        got = {}
        for chunk in (64, 0):
            mean, var = G.gp_posterior(gm, Z[:nq], chunk=chunk)
            got[chunk] = (mean.cpu().numpy(), var.cpu().numpy())
            wm, wv = worst_posterior(m, ref, *got[chunk], rows=slice(0, nq))
            print("  n %3d ds %d da %d %-6s nq %3d chunk %2d: mean %.3f, var %.3f of the tolerance" % (n, ds, da, kind, nq, chunk, wm, wv))
            assert wm <= 1.0 and wv <= 1.0
        assert np.array_equal(got[64][0], got[0][0]) and np.array_equal(got[64][1], got[0][1])     # columns are independent: the chunk does not matter


def test_gp_posterior_sums_all_entries_of_a_nonsymmetric_inverse(G):
    """The bound holds on an inverse perturbed by 1e-3 per entry; the reference that reads only one triangle of it (mirrored), or with its
    rows from 64 on dropped (a second row block that is not visited), misses the same bound by more than 1e3.  The matrix TRANSPOSED
    cannot serve as a control: a quadratic form does not change under it (measured: 2e-5 of the tolerance)."""
    m = model_data(130, 2, 1, "nonsym")
    gm = device_model(G, m)
    Z = queries(m, 65)
    ref = R.posterior(m, Z)
    mean, var = (t.cpu().numpy() for t in G.gp_posterior(gm, Z, chunk=64))
    wm, wv = worst_posterior(m, ref, mean, var)
    print("  non-symmetric inverse: mean %.3f, var %.3f of the tolerance" % (wm, wv))
    assert wm <= 1.0 and wv <= 1.0
    for wrong in (dict(triangle_only=True), dict(drop_rows_from=64)):
        bad = R.posterior(m, Z, **wrong)
        miss = float((np.abs(var - f64(bad["s2"])) / var_tol(m, ref)).max())
        print("  control %s: misses by %.3g tolerances" % (wrong, miss))
        assert miss > 1e3


def test_gp_posterior_sparse_model(G):
    """(Z, alpha, Q) of SparseGPState through SparseDynamics: M = 70 inducing points, two hyper-parameter groups."""
    from gaussian_process_mpc_amd.synth import synth_problem
    pb = synth_problem(7, 300, 2, 1, 3, 2, sigma_n=0.05)
    idx = np.random.default_rng(5).choice(300, size=70, replace=False)
    dyn = G.SparseDynamics(2, 1, pb["X"][idx])
    for a, g in enumerate(dyn.gpr_err):
        g.set_lambdas(pb["lambdas"][a])
        g.set_sigma_f(0.9 + 0.3 * a)
        g.set_sigma_n(0.05)
    dyn.append_train_data(pb["X"][:, :2], pb["X"][:, 2:], pb["Y"])
    gm = G.GPModel.from_dynamics(dyn)
    assert gm.n == 70 and gm.c.gp_stride == 70 * 70
    m = dict(X=gm.X.cpu().numpy(), beta=gm.beta.cpu().numpy(), Kinv=gm.Kinv.cpu().numpy(), lam=gm.lambdas, sf=gm.sigma_f)
    Z = queries(m, 65)
    ref = R.posterior(m, Z)
    mean, var = (t.cpu().numpy() for t in G.gp_posterior(dyn, Z, chunk=64))
    wm, wv = worst_posterior(m, ref, mean, var)
    print("  sparse model: mean %.3f, var %.3f of the tolerance" % (wm, wv))
    assert wm <= 1.0 and wv <= 1.0
    # ... and it is the posterior the existing entry point gives for each group (gpmpc_predict through SparseGPState.predict), to rounding
    for cols, st in dyn._ensure_groups():
        pm, pc = st.predict(Z)
        # (two float64 routes to the same sums: each within its budget of the long double value, so within twice that of each other)
        assert np.all(np.abs(mean[:, cols] - pm.cpu().numpy()) <= 2.0 * TOL * f64(ref["m_abs"])[:, cols])
        assert np.all(np.abs(var[:, cols[0]] - np.diagonal(pc.cpu().numpy())) <= 2.0 * var_tol(m, ref)[:, cols[0]])


# ------------------------------------------------------------------------------------------------------------------ noise
def test_particle_noise(G):
    for (P, nn, t, seed, call) in [(70, 3, 2, 5, 1), (1, 2, 0, 0, 0), (300, 16, 7, (3 << 32) + 9, 4), (5, 1, 1, 2 ** 64 - 1, 2 ** 32 - 1)]:
        a = G.particle_noise(P, nn, t, seed, call).cpu().numpy()
        ref = R.normals(seed, call, t, P, nn)
        print("  noise P %d n %d t %d: worst %.2e" % (P, nn, t, np.abs(a - ref).max()))
        assert np.abs(a - ref).max() <= 1e-12
        assert np.array_equal(a, G.particle_noise(P, nn, t, seed, call).cpu().numpy())
        if P > 4:                                                         # a value does not depend on P or on the normals asked for
            assert np.array_equal(a[:4], G.particle_noise(4, nn, t, seed, call).cpu().numpy())
            assert np.array_equal(a[:, :1], G.particle_noise(P, 1, t, seed, call).cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ step and rollout
H, B = 3, 2


def roll_inputs(m):
    ds, da, _ = R.dims(m)
    rng = np.random.default_rng(17)
    return rng.uniform(-0.8, 0.8, (B, ds)), rng.uniform(-0.8, 0.8, (B, H, da))


@pytest.mark.parametrize("P", [1, 70])
@pytest.mark.parametrize("case", ["pergp", "shared_nominal_noise"])
def test_rollout_is_the_chain_and_each_step_is_the_reference(G, case, P):
    m = model_data(70, 2, 1, "pergp") if case == "pergp" else model_data(70, 2, 1, "shared", process_var=True, nominal=True)
    ds, da, D = R.dims(m)
    gm = device_model(G, m)
    x0, U = roll_inputs(m)
    seed, call = 11, 2
    r = G.particle_rollout(gm, x0, U, particles=P, seed=seed, call_index=call, chunk=64)          # B P = 140: three chunks
    X = r["particles"].permute(2, 0, 1, 3).contiguous()                                            # (H+1, B, P, ds)
    r0 = G.particle_rollout(gm, x0, U, particles=P, seed=seed, call_index=call)                    # the default chunk: the same bits
    assert torch.equal(r["particles"], r0["particles"]) and torch.equal(r["mean"], r0["mean"]) and same_bits(r["cov"], r0["cov"])
    assert bool(torch.isnan(r["cov"]).all()) == (P == 1)
    Xh = X.cpu().numpy()
    # the initial draw: x0 + L eps, a few roundings
    ref0 = R.initial(m, x0, P, seed, call)
    assert np.abs(Xh[0] - ref0).max() <= 8 * ULP * np.abs(ref0).max()
    assert np.allclose(Xh[0, 0] - x0[0], Xh[0, 1] - x0[1], rtol=0, atol=1e-15)   # plans share draws
    worst = 0.0
    for t in range(1, H + 1):
        eps = G.particle_noise(P, da + ds, t, seed, call)
        nxt, mean, var = G.particle_step(gm, X[t - 1], U[:, t - 1], eps, chunk=64, return_moments=True)
        assert torch.equal(nxt, X[t]), "step %d of the rollout is not the chain of noise + step calls" % t                   # no tolerance
        ref = R.step(m, Xh[t - 1], U[:, t - 1], eps.cpu().numpy())
        s2 = f64(ref["s2"])
        assert s2.min() > 0.0, "the reference clamps a particle: choose other inputs"
        e = eps.cpu().numpy()[None, :, da:]
        tol = TOL * f64(ref["m_abs"]) + np.abs(e) * (TOL * f64(ref["q_abs"]) + 2.0 * ULP * (np.asarray(m["sf"]) ** 2 + R.noise_model(m)[2])) \
            / (2.0 * np.sqrt(s2)) + 4.0 * ULP * np.abs(f64(ref["next"]))
        w = float((np.abs(nxt.cpu().numpy() - f64(ref["next"])) / tol).max())
        wm = float((np.abs(mean.cpu().numpy() - f64(ref["m"])) / (TOL * f64(ref["m_abs"]))).max())
        worst = max(worst, w, wm)
        print("  %s P %d step %d: draw %.3f, mean %.3f of the tolerance; min s2 %.2e" % (case, P, t, w, wm, s2.min()))
    assert worst <= 1.0
    assert int(r["clamped"].sum().item()) == 0


def test_negative_variance_is_returned_unclamped_and_counted(G):
    """Kinv scaled by 1 + 1e-3 and a query AT a training point (sigma_n = 0.01): s2 = sf^2 - 1.001 q < 0 deterministically.  out_var is
    negative, the draw equals the mean, and the statistics count every particle of that step."""
    base = model_data(70, 2, 1, "pergp", seed=9, sn=0.01)
    m = dict(base, Kinv=base["Kinv"] * (1.0 + 1e-3), init_cov=np.zeros((2, 2)), action_var=np.zeros(1), process_var=np.zeros(2))
    gm = device_model(G, m)
    P, j = 5, 7
    x_prev = np.tile(m["X"][j, :2], (1, P, 1))
    eps = G.particle_noise(P, 3, 1, 1, 0)
    nxt, mean, var = G.particle_step(gm, x_prev, m["X"][j, 2:][None], eps, return_moments=True)
    ref = R.posterior(m, m["X"][j][None])
    assert f64(ref["s2"]).max() < 0.0
    assert float(var.max().item()) < 0.0 and torch.equal(nxt, mean)
    assert np.abs(var.cpu().numpy()[0, 0] - f64(ref["s2"][0])).max() <= float(var_tol(m, ref).max())
    # the rollout from that point, exactly known (a zero init_cov: every pivot zero): step 1 clamps every particle, and says so
    U = np.zeros((1, 2, 1))
    U[0, 0] = m["X"][j, 2:]
    r = G.particle_rollout(gm, m["X"][j, :2], U, particles=P, seed=1)
    assert torch.equal(r["particles"][0, :, 0], torch.as_tensor(x_prev[0], device="cuda"))
    assert int(r["clamped"][0, 0].item()) == P
    assert torch.equal(r["particles"][0, :, 1], mean[0])


# ------------------------------------------------------------------------------------------------------------------ stats
def test_particle_stats(G):
    m = model_data(70, 2, 1, "pergp")
    gm = device_model(G, m)
    x0, U = roll_inputs(m)
    P = 300                                                               # more particles than threads: two per thread, then the fold
    A = np.array([[1.0, 0.0], [0.3, -0.8]])
    plain = G.particle_rollout(gm, x0, U, particles=P, seed=4)
    X = plain["particles"].permute(2, 0, 1, 3).contiguous()
    Xh = X.cpu().numpy()
    # b: per row, the midpoint of the widest gap around the 80 % quantile of a . x over all steps and plans -- no value within 1e-9 of it
    g0 = f64(R.violations(Xh, A, np.zeros(2)))
    b = np.empty(2)
    for r_ in range(2):
        v = np.sort(g0[1:, ..., r_].reshape(-1))
        k = int(0.8 * v.size)
        k = k - 3 + int(np.argmax(np.diff(v[k - 3:k + 4])))
        b[r_] = 0.5 * (v[k] + v[k + 1])
    g = f64(R.violations(Xh, A, b))
    assert np.abs(g).min() >= 1e-9, "a particle sits on a constraint boundary: no case may be left out"
    sc = G.StateConstraints(A, b, kappa=0.0)
    r = G.particle_rollout(gm, x0, U, particles=P, seed=4, constraints=sc)
    assert torch.equal(r["particles"], plain["particles"])
    ref = R.stats(Xh)
    em = np.abs(r["mean"].cpu().numpy() - f64(ref["mean"])) / (TOL * f64(ref["mean_abs"]) / P)
    ec = np.abs(r["cov"].cpu().numpy() - f64(ref["cov"])) / (TOL * f64(ref["cov_abs"]) / (P - 1))
    print("  stats: mean %.3f, cov %.3f of the tolerance" % (em.max(), ec.max()))
    assert em.max() <= 1.0 and ec.max() <= 1.0
    cov = r["cov"]
    assert torch.equal(cov, cov.transpose(-1, -2))
    viol = np.moveaxis((g > 0).sum(axis=2) / P, 0, 1)                     # (B, T, rows)
    joint = (g[1:] > 0).any(axis=(0, 3)).sum(axis=1) / P                  # (B,)
    assert np.array_equal(r["violation"].cpu().numpy(), viol) and np.array_equal(r["joint_violation"].cpu().numpy(), joint)
    assert np.any((viol[:, 1:] > 0.0) & (viol[:, 1:] < 1.0)) and np.any((joint > 0.0) & (joint < 1.0))     # (a bound that splits the particles)
    assert np.all(r["joint_violation"].cpu().numpy() >= r["violation"].cpu().numpy()[:, 1:].max(axis=(1, 2)))
    # the stand-alone entry point on the same particles, and the same bits twice
    s1 = G.particle_stats(X, constraints=sc)
    s2 = G.particle_stats(X, constraints=sc)
    for k in ("mean", "cov", "violation", "joint_violation"):
        assert torch.equal(s1[k], s2[k]) and torch.equal(s1[k], r[k]), k
    var = torch.ones_like(X)
    var[2, 1, :7, 1] = -1.0
    assert G.particle_stats(X, var=var)["clamped"].cpu().numpy().tolist() == [[0, 0, 0, 0], [0, 0, 7, 0]]


# ------------------------------------------------------------------------------------------------------------------ Python surface
def _dynamics(G, kind):
    from gaussian_process_mpc_amd.synth import synth_problem
    pb = synth_problem(3, 90, 2, 1, 3, 2, sigma_n=0.05)
    nominal = G.LinearNominalModel.identity(2, 1) if kind == "nominal" else None
    if kind == "sparse":
        dyn = G.SparseDynamics(2, 1, pb["X"][np.random.default_rng(5).choice(90, size=40, replace=False)])
    else:
        dyn = G.Dynamics(2, 1, nominal_models=nominal)
    for a, g in enumerate(dyn.gpr_err):
        g.set_lambdas(pb["lambdas"][a] if kind != "windowed" else pb["lambdas"][0])
        g.set_sigma_f(1.0 if kind == "windowed" else 0.8 + 0.3 * a)
        g.set_sigma_n(0.05)
    if kind == "windowed":
        dyn.max_train = 70
    dyn.append_train_data(pb["X"][:, :2], pb["X"][:, 2:], pb["Y"])
    if kind == "windowed":                                                # one more observation: it replaces a row of the window
        dyn.append_train_data(np.array([0.1, 0.2]), np.array([0.3]), np.array([0.12, 0.25]), incremental=True)
    dyn.set_noise_model(init_cov=np.diag([0.02, 0.01]), action_var=[0.01], process_var="sigma_n" if kind == "dense" else None)
    return dyn, pb


@pytest.mark.parametrize("kind", ["dense", "windowed", "nominal", "sparse"])
def test_dynamics_particle_rollout(G, kind):
    """The model a Dynamics hands over is the one its rollout uses: step 1 of the moment-matched rollout is exact, so the particle moments
    agree with it within 4 Monte-Carlo standard errors; the rollout itself is untouched by the particle run."""
    dyn, pb = _dynamics(G, kind)
    P = 4096
    before = dyn.rollout(pb["x0"], pb["U"])
    r = dyn.particle_rollout(pb["x0"], pb["U"], particles=P, seed=2)
    after = dyn.rollout(pb["x0"], pb["U"])
    assert torch.equal(before["means"], after["means"]) and torch.equal(before["vars"], after["vars"])
    gm = r["model"]
    assert gm.n == {"dense": 90, "windowed": 70, "nominal": 90, "sparse": 40}[kind]
    assert (gm.nominal is not None) == (kind == "nominal") and (kind == "windowed" or gm.c.gp_stride == gm.n ** 2)
    assert r["particles"].shape == (2, P, 4, 2) and int(r["clamped"].sum().item()) == 0
    X1 = r["particles"][:, :, 1].cpu().numpy()
    d = X1 - X1.mean(axis=1, keepdims=True)
    v = (d ** 2).sum(axis=1) / (P - 1)
    z_mean = (r["mean"][:, 1].cpu().numpy() - before["means"][:, 1].cpu().numpy()) / np.sqrt(v / P)
    z_var = (v - before["vars"][:, 1].cpu().numpy()) / np.sqrt(((d ** 4).mean(axis=1) - v ** 2) / P)
    print("  %s: z(mean) %s z(var) %s" % (kind, np.round(z_mean, 2).tolist(), np.round(z_var, 2).tolist()))
    assert np.abs(z_mean).max() <= 4.0 and np.abs(z_var).max() <= 4.0
    np.testing.assert_allclose(r["cov"][:, 1].cpu().numpy()[:, [0, 1], [0, 1]], v, rtol=1e-12)
    for k in ("mean", "cov"):
        assert bool(torch.isfinite(r[k]).all())


def test_validate_plan_on_c1(G):
    """RiskSensitiveMPC.validate_plan on the c1 problem of tests/test_gpu_constraints.py: finite tables, and the step-1 differences below
    4 standard errors (the GPU twin of the host pin)."""
    from gaussian_process_mpc_amd.synth import synth_problem
    pb = synth_problem(1, 100, 2, 2, 10, 64)
    ds, da, Hh = 2, 2, 10
    mpc = G.RiskSensitiveMPC(1e-5, Hh, ds, da, pb["Q"], pb["R"])
    for a, g in enumerate(mpc.dynamics.gpr_err):
        g.set_lambdas(pb["lambdas"][a])
        g.set_sigma_n(float(pb["sigma_n"][a]))
        g.set_sigma_f(1.0)
    mpc.dynamics.append_train_data(pb["X"][:, :ds], pb["X"][:, ds:], pb["Y"])
    mpc.set_state_constraints(np.array([[1.0, 0.0]]), [0.5], prob=0.95)
    v = mpc.validate_plan(U=pb["U"][0], x0=pb["x0"][0], particles=4096, seed=0)
    for k in ("mean_mm", "var_mm", "mean_mc", "var_mc", "z_mean", "z_var", "satisfaction"):
        assert np.all(np.isfinite(v[k])), k
    assert v["mean_mc"].shape == (Hh + 1, ds) and v["satisfaction"].shape == (Hh, 1) and v["requested"].shape == (1,)
    assert abs(v["requested"][0] - 0.95) < 1e-12 and 0.0 <= v["joint_satisfaction"] <= v["satisfaction"].min() <= 1.0
    assert np.isfinite(v["stage_cost"]) and v["stage_cost"] > 0
    print("  validate_plan: step 1 z(mean) %s z(var) %s; worst over the horizon %.2f / %.2f; clamped %d"
          % (np.round(v["z_mean"][1], 2), np.round(v["z_var"][1], 2), np.abs(v["z_mean"]).max(), np.abs(v["z_var"]).max(), v["clamped"].sum()))
    assert np.abs(v["z_mean"][1]).max() <= 4.0 and np.abs(v["z_var"][1]).max() <= 4.0
    mpc.full_covariance = True
    mpc.clear_state_constraints()
    vf = mpc.validate_plan(U=pb["U"][0], x0=pb["x0"][0], particles=1024, seed=0)
    assert vf["cov_mm"].shape == (Hh + 1, ds, ds) and np.all(np.isfinite(vf["cov_mc"])) and "satisfaction" not in vf
