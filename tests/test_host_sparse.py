"""Holds tests/sparse_reference.py itself and everything of the sparse GP (FITC inducing points) that needs no device (CPU):

  * the whitened formulas ARE the direct FITC definition (mpmath, 100 bits, M = 8, N = 20, to 1e-15 relative);
  * with Z = X and jitter = 0 they give the dense GP's beta and Ky_inv and, through the restated rollout, the pinned oracle's own
    rollout, cost and gradient (N = 40) to 1e-12;
  * a rank-one append equals the batch fit in extended precision to 1e-13;
  * the two conditions that make the end-to-end GPU tolerances of tests/test_gpu_sparse.py mean something: the honest float64
    evaluation sits ten-fold under each of them on each end-to-end case, and three deliberate mistakes (a dropped data row, a dropped
    inducing point, sigma_f^2 for sigma_f^2 + sigma_n^2 in Lambda) move some output by at least 100 times its tolerance;
  * the C ABI: names, struct-free signatures, workspace sizes, the refusals that come before any launch; argument errors of the
    Python surface that come before the device is needed; select_inducing."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import sparse_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the end-to-end tolerances of tests/test_gpu_sparse.py: (rtol, atol) -- the project's figures (__graft_entry__.smoke)
E2E_TOL = {"means": (1e-5, 1e-9), "vars": (1e-4, 1e-12), "cost": (1e-6, 0.0), "grad": (1e-4, 1e-7), "covs": (1e-4, 1e-12)}
E2E_CASES = {"ds2": dict(N=300, ds=2, M=32, lam_range=(2.0, 6.0)), "ds4": dict(N=200, ds=4, M=48, lam_range=(0.5, 1.5))}


def e2e_problem(tag):
    """The end-to-end cases of the GPU tests: synth_problem(7, N, ds, 1, 5, 2) and Z = X[default_rng(5).choice(N, M, replace=False)]."""
    from gaussian_process_mpc_amd.synth import synth_problem
    c = E2E_CASES[tag]
    pb = synth_problem(7, c["N"], c["ds"], 1, 5, 2, lam_range=c["lam_range"])
    idx = np.random.default_rng(5).choice(c["N"], size=c["M"], replace=False)
    return pb, np.ascontiguousarray(pb["X"][idx])


def _rollouts(pb, Z, alpha, Q, fullcov=False):
    return [R.rollout(Z, alpha, Q, pb["lambdas"], pb["sigma_f"], pb["H"], pb["x0"][b], pb["U"][b], pb["Q"], pb["R"], -1.0, fullcov=fullcov)
            for b in range(pb["B"])]


@functools.lru_cache(maxsize=None)
def _e2e_reference(tag, fullcov=False):
    pb, Z = e2e_problem(tag)
    alpha, Q = R.fit_bundle(pb, Z)
    return pb, Z, _rollouts(pb, Z, alpha, Q, fullcov)


def _worst_ratio(got, ref, keys):
    """max over keys and entries of |got - ref| / (atol + rtol |ref|)."""
    w = 0.0
    for k in keys:
        rtol, atol = E2E_TOL[k]
        g, r = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        w = max(w, float(np.max(np.abs(g - r) / (atol + rtol * np.abs(r)))))
    return w


# ------------------------------------------------------------------------------------------------------------------ the mathematics
def test_whitened_equals_direct_fitc_mpmath():
    import mpmath as mp
    with mp.workprec(100):
        pr = R.problem(3, 20, 8, 3, 2)
        w = R.fit(pr["X"], pr["Y"], pr["Z"], pr["lam"], pr["sf"], pr["noise"], pr["jitter"], prec=R.MP)
        d = R.direct_fitc(pr["X"], pr["Y"], pr["Z"], pr["lam"], pr["sf"], pr["noise"], pr["jitter"], prec=R.MP)
        for k in ("alpha", "Q"):
            rel = R.err(w[k], d[k]) / R.max_abs(d[k])
            print("  whitened against direct FITC, %s: %.2e relative" % (k, rel))
            assert rel <= 1e-15
        assert R.err(w["Lambda"], d["Lambda"]) <= 1e-15 * R.max_abs(d["Lambda"])


@functools.lru_cache(maxsize=None)
def _dense_problem():
    from gaussian_process_mpc_amd.synth import synth_problem
    return synth_problem(7, 40, 2, 1, 5, 2, lam_range=(0.3, 0.6))


@pytest.mark.parametrize("prec", [R.DEFAULT, np.float64], ids=["extended", "float64"])
def test_inducing_at_the_data_is_the_dense_gp(prec):
    """Z = X, jitter = 0: alpha = Ky^-1 y and Q = Ky^-1, to 1e-12 of the largest entry, in extended precision and in float64."""
    pb = _dense_problem()
    for a in range(pb["ds"]):
        lam, sf, noise = pb["lambdas"][a], float(pb["sigma_f"][a]), float(pb["sigma_n"][a]) ** 2
        f = R.fit(pb["X"], pb["Y"][:, a], pb["X"], lam, sf, noise, 0.0, prec=prec)
        Ky = R.kmm(pb["X"], lam, sf, noise)                                  # (extended precision: the dense GP's own matrices)
        Kinv = R.inv_spd(Ky)
        beta = Kinv @ R.cast(pb["Y"][:, a])
        e_b, e_k = R.err(f["alpha"][:, 0], beta) / R.max_abs(beta), R.err(f["Q"], Kinv) / R.max_abs(Kinv)
        print("  Z = X, GP %d: beta %.2e, Ky_inv %.2e relative" % (a, e_b, e_k))
        assert e_b <= 1e-12 and e_k <= 1e-12


def test_inducing_at_the_data_is_the_oracle_rollout():
    """The restated rollout on (Z = X, alpha, Q) is the pinned oracle's objective_and_gradient on the dense GP, to 1e-12."""
    from oracle import gpmpc_oracle as O
    pb = _dense_problem()
    alpha, Q = R.fit_bundle(pb, pb["X"], jitter=0.0)
    Kinv = np.stack([R.to_f64(R.inv_spd(R.kmm(pb["X"], pb["lambdas"][a], float(pb["sigma_f"][a]), float(pb["sigma_n"][a]) ** 2)))
                     for a in range(pb["ds"])])
    gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"], Ky_inv=Kinv)
    for b in range(pb["B"]):
        o = O.objective_and_gradient(gp, pb["H"], pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], -1.0, mode="o2")
        r = R.rollout(pb["X"], alpha, Q, pb["lambdas"], pb["sigma_f"], pb["H"], pb["x0"][b], pb["U"][b], pb["Q"], pb["R"], -1.0)
        for k in ("means", "vars", "grad"):
            e = np.abs(r[k] - o[k]).max() / np.abs(o[k]).max()
            print("  Z = X rollout %d, %s: %.2e of the largest" % (b, k, e))
            assert e <= 1e-12
        assert abs(r["cost"] - o["cost"]) <= 1e-12 * abs(o["cost"])


def test_append_equals_batch_extended_precision():
    """20 rank-one appends after a fit on N - 20 rows against the fit on all N rows, to 1e-13 of the largest entry."""
    pr = R.problem(11, 120, 24, 3, 2)
    n0 = pr["n"] - 20
    args = (pr["lam"], pr["sf"], pr["noise"])
    full = R.fit(pr["X"], pr["Y"], pr["Z"], *args, pr["jitter"], W=pr["W"])
    st = R.fit(pr["X"][:n0], pr["Y"][:n0], pr["Z"], *args, pr["jitter"], W=pr["W"])
    for i in range(n0, pr["n"]):
        st = R.append(pr["X"][i], pr["Y"][i], pr["Z"], pr["W"], *args, st["G"], st["r"], st["Binv"], st["Q"])
    for k in ("G", "r", "Binv", "Q", "alpha"):
        rel = R.err(st[k], full[k]) / R.max_abs(full[k])
        print("  append against batch, %s: %.2e relative" % (k, rel))
        assert rel <= 1e-13


# ------------------------------------------------------------------------------------------------------------------ tolerances mean something
@pytest.mark.parametrize("tag", sorted(E2E_CASES))
@pytest.mark.parametrize("fullcov", [False, True], ids=["diag", "fullcov"])
def test_float64_sits_tenfold_under_the_end_to_end_tolerances(tag, fullcov):
    pb, Z, ref = _e2e_reference(tag, fullcov)
    alpha, Q = R.fit_bundle(pb, Z, prec=np.float64)
    keys = ("means", "covs" if fullcov else "vars", "cost", "grad")
    worst = max(_worst_ratio(g, r, keys) for g, r in zip(_rollouts(pb, Z, alpha, Q, fullcov), ref))
    print("  %s %s: float64 restatement at %.3g of the end-to-end tolerances" % (tag, "fullcov" if fullcov else "diag", worst))
    assert worst <= 0.1


@pytest.mark.parametrize("mistake", ["data_row", "inducing_point", "lambda_without_noise"])
def test_mistakes_move_the_outputs_hundredfold(mistake):
    pb, Z, ref = _e2e_reference("ds2")
    if mistake == "data_row":
        pb2 = dict(pb, X=pb["X"][1:], Y=pb["Y"][1:])
        alpha, Q = R.fit_bundle(pb2, Z)
    elif mistake == "inducing_point":
        alpha, Q = R.fit_bundle(pb, Z[:-1])
        Z = Z[:-1]
    else:
        alpha, Q = R.fit_bundle(pb, Z, lambda_noise=False)
    worst = max(_worst_ratio(g, r, ("means", "vars", "cost", "grad")) for g, r in zip(_rollouts(pb, Z, alpha, Q), ref))
    print("  %s: moves an output by %.3g times its tolerance" % (mistake, worst))
    assert worst >= 100.0


def test_allowance_rule():
    a = np.array([1.0, -3.0], dtype=R.LD)
    assert R.allowance(a, np.array([1.0, -3.0])) == 1e-13 * 3.0
    assert R.allowance(a, np.array([1.0 + 1e-10, -3.0])) == pytest.approx(8e-10, rel=1e-3)


# ------------------------------------------------------------------------------------------------------------------ ABI and Python surface
NAMES = ["gpmpc_sparse_accumulate_workspace_bytes", "gpmpc_sparse_accumulate", "gpmpc_sparse_finish_workspace_bytes", "gpmpc_sparse_finish",
         "gpmpc_sparse_append_workspace_bytes", "gpmpc_sparse_append", "gpmpc_sparse_set_form"]
E_ARG, E_WORKSPACE = -1, -4


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_mpc_amd import _lib
    return _lib.lib()


def test_abi_names_and_struct_free_signatures(L):
    from gaussian_process_mpc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    plain = (ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t, ctypes.POINTER(ctypes.c_double))
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        res, args = _lib.SIGNATURES[name]
        assert res in (ctypes.c_int, ctypes.c_size_t)
        assert all(a in plain for a in args), name                        # no struct travels through these entry points
        assert getattr(L, name) is not None
        n_decl = len(re.search(r"\b%s\s*\((.*?)\);" % name, hdr, flags=re.S).group(1).split(","))
        assert n_decl == len(args), (name, n_decl, len(args))


def test_workspace_sizes(L):
    acc = L.gpmpc_sparse_accumulate_workspace_bytes
    assert acc(10, 3, 32, 2, 64) == acc(10 ** 6, 8, 32, 7, 64)            # (M, chunk) only: not n, D, n_targets
    assert acc(10, 3, 32, 2, 0) == acc(10, 3, 32, 2, 4096)                # 0: the default chunk
    assert acc(10, 3, 32, 2, 64) >= 8 * (32 * 64 + 64 + 64)               # V, one row block of partial sums, 1 / Lambda
    assert acc(10, 3, 32, 2, 100) == 0 and acc(10, 3, 0, 2, 64) == 0
    assert L.gpmpc_sparse_finish_workspace_bytes(33, 2) >= 8 * (33 * 33 + 33 * 2)
    assert L.gpmpc_sparse_append_workspace_bytes(33, 2) >= 8 * (3 * 33 + 33 * 2)


def test_refusals_before_any_launch(L):
    """Every refusal is decided on the host, from sizes and pointers: GPMPC_E_ARG with a text (no device is touched: this runs without one)."""
    from gaussian_process_mpc_amd._lib import host_doubles, MAX_D, MAX_DS
    lam = host_doubles(np.ones(8))[1]
    p = ctypes.c_void_p(4096)                                               # never dereferenced: every call below is refused first

    def acc(n=10, D=3, M=8, nt=2, X=p, Y=p, ld_y=2, Z=p, W=p, ld_w=8, lam=lam, chunk=64, G=p, r=p, st=p, ws=p, nb=1 << 30):
        return L.gpmpc_sparse_accumulate(n, D, M, nt, X, Y, ld_y, Z, W, ld_w, lam, 1.0, 1e-2, chunk, 0, G, r, st, ws, nb, None)

    cases = {"n < 1": dict(n=0), "M": dict(M=0), "M (": dict(M=8193, ld_w=8193), "D outside": dict(D=MAX_D + 1), "n_targets": dict(nt=0),
             "n_targets outside": dict(nt=MAX_DS + 1, ld_y=MAX_DS + 1), "chunk": dict(chunk=96), "chunk must": dict(chunk=-64),
             "ld_y": dict(ld_y=1), "ld_w": dict(ld_w=7), "NULL": dict(X=None), "NULL pointer": dict(st=None)}
    for text, kw in cases.items():
        assert acc(**kw) == E_ARG, kw
        assert text in L.gpmpc_last_error().decode(), (kw, L.gpmpc_last_error())
    assert acc(nb=L.gpmpc_sparse_accumulate_workspace_bytes(10, 3, 8, 2, 64) - 1) == E_WORKSPACE

    def fin(M=8, nt=2, W=p, ld_w=8, Binv=p, r=p, alpha=p, Q=p, ws=p, nb=1 << 30):
        return L.gpmpc_sparse_finish(M, nt, W, ld_w, Binv, r, alpha, Q, ws, nb, None)

    for kw in (dict(M=0), dict(nt=9), dict(ld_w=7), dict(Binv=None), dict(Q=None)):
        assert fin(**kw) == E_ARG, kw
        assert "gpmpc_sparse_finish" in L.gpmpc_last_error().decode()
    assert fin(nb=L.gpmpc_sparse_finish_workspace_bytes(8, 2) - 1) == E_WORKSPACE

    def app(D=3, M=8, nt=2, x=p, y=p, Z=p, W=p, ld_w=8, lam=lam, G=p, r=p, Binv=p, Q=p, alpha=p, st=p, ws=p, nb=1 << 30):
        return L.gpmpc_sparse_append(D, M, nt, x, y, Z, W, ld_w, lam, 1.0, 1e-2, G, r, Binv, Q, alpha, st, ws, nb, None)

    for kw in (dict(D=0), dict(D=9), dict(M=0), dict(nt=0), dict(ld_w=7), dict(x=None), dict(alpha=None), dict(lam=None)):
        assert app(**kw) == E_ARG, kw
        assert "gpmpc_sparse_append" in L.gpmpc_last_error().decode()
    assert app(nb=L.gpmpc_sparse_append_workspace_bytes(8, 2) - 1) == E_WORKSPACE
    # the form of the two products, FMA (0) or MFMA (1): -1 asks; a set returns the form before it; anything else is refused and changes nothing
    cur = L.gpmpc_sparse_set_form(-1)
    assert cur in (0, 1) and L.gpmpc_sparse_set_form(1 - cur) == cur and L.gpmpc_sparse_set_form(7) == E_ARG
    assert "gpmpc_sparse_set_form" in L.gpmpc_last_error().decode() and L.gpmpc_sparse_set_form(cur) == 1 - cur and L.gpmpc_sparse_set_form(-1) == cur


def test_sparse_dynamics_argument_errors(L):
    """Argument errors come before the device is needed."""
    import gaussian_process_mpc_amd as g
    Z = np.zeros((4, 3))
    with pytest.raises(ValueError, match="inducing points"):
        g.SparseDynamics(2, 1, np.zeros((4, 2)))
    with pytest.raises(ValueError, match="inducing points"):
        g.SparseDynamics(2, 1, np.zeros((0, 3)))
    with pytest.raises(ValueError, match="finite"):
        g.SparseDynamics(2, 1, np.full((4, 3), np.nan))
    with pytest.raises(ValueError, match="LinearNominalModel"):
        g.SparseDynamics(2, 1, Z, nominal_models=[lambda x: x, lambda x: x])
    with pytest.raises(ValueError, match="chunk"):
        g.SparseDynamics(2, 1, Z, chunk=100)
    with pytest.raises(ValueError, match="jitter"):
        g.SparseDynamics(2, 1, Z, jitter=-1.0)


def test_select_inducing():
    import gaussian_process_mpc_amd as g
    rng = np.random.default_rng(0)
    X = rng.uniform(-2, 2, (200, 3))
    lam = np.array([1.0, 4.0, 0.25])
    Z, idx = g.select_inducing(X, 16, lam, return_index=True)
    assert Z.shape == (16, 3) and len(set(idx.tolist())) == 16 and np.array_equal(Z, X[idx])
    # greedy farthest point: every pick is the row farthest (lambda-metric) from the picks before it
    for k in range(1, 16):
        d = np.min(((X[:, None, :] - X[idx[:k]][None, :, :]) ** 2 / lam).sum(axis=2), axis=1)
        assert idx[k] == int(np.argmax(d))
    # ... so it covers the data better than a random draw: the largest distance of a row to its nearest inducing point is smaller
    def cover(Zs):
        return np.max(np.min(((X[:, None, :] - Zs[None, :, :]) ** 2 / lam).sum(axis=2), axis=1))
    Zr = g.select_inducing(X, 16, lam, method="random", seed=3)
    assert np.array_equal(Zr, g.select_inducing(X, 16, lam, method="random", seed=3)) and cover(Z) < cover(Zr)
    assert np.array_equal(g.select_inducing(X, 200, lam)[np.argsort(g.select_inducing(X, 200, lam, return_index=True)[1])], X)
    for bad in (dict(M=0), dict(M=201), dict(method="kmeans")):
        with pytest.raises(ValueError):
            g.select_inducing(X, **dict(dict(M=4, lambdas=lam), **bad))
