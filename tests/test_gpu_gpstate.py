"""The GP-state entry points of the C ABI (gpmpc_build_ky, gpmpc_predict, gpmpc_matvec, gpmpc_kinv_append, gpmpc_gp_append,
gpmpc_kinv_remove, gpmpc_gp_replace, gpmpc_ml_grad) against the extended-precision restatement of tests/gpstate_reference.py, over a
ladder of sizes that puts one point either side of every tile edge of their kernels, with a genuinely NON-symmetric Ky_inv: a
transposed index (K k for K^T k, K[:, p] for K[p, :], K* K^T for K* K) moves these results by percents.

Tolerances (tests/test_host_gpstate.py holds the conditions they rest on):
  * Schur updates: 1e-12 of the largest element -- the project's figure for this operation (test_gp_replace_abi_padded_buffers_...);
    a plain float64 evaluation of the same formulas stays under 1e-13 on every case of the ladder.
  * dot products: 1e-12 x the sum of absolute terms -- above the worst case of ANY summation order at these sizes (strided partial
    sums of at most n^2 / 256 + 20 additions at 1.1e-16: 1.2e-13 at n = 520), while one missing term is about 1 / n^2 >= 4e-6 of it.
  * kernel-matrix entries: rtol 1e-12 (test_gpr_matrices_and_predict); the exponent is at most 92 with these inputs and its rounding
    (D + 3) eps 92 = 1.1e-13.
Every workspace is followed by a 4096-byte guard band inside the test's own allocation and is handed over at exactly
*_workspace_bytes(...): an overrun shows as changed bytes."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gpstate_reference as R

pytestmark = pytest.mark.gpu

TOL = 1e-12
GUARD, PATTERN = 4096, 0xA5
E_WORKSPACE = -4
P_LADDER = (1, 7, 8, 9, 17)
_WORST = {}


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    yield g
    print("\n  worst error / tolerance per entry point: " + ", ".join("%s %.3f" % kv for kv in sorted(_WORST.items())))


@functools.lru_cache(maxsize=None)
def _problem(n, D):
    return R.problem(R.seed_of(n, D), n, D)


def _note(name, ratio):
    _WORST[name] = max(_WORST.get(name, 0.0), float(ratio))
    return float(ratio)


def _L():
    from gaussian_process_mpc_amd._lib import lib
    return lib()


def _sp():
    from gaussian_process_mpc_amd._lib import stream_ptr
    return stream_ptr()


def _check(rc, what):
    from gaussian_process_mpc_amd._lib import check
    check(rc, what)


def _lp(lam):
    from gaussian_process_mpc_amd._lib import host_doubles
    return host_doubles(np.array(lam))


def _dev(a):
    return torch.tensor(np.array(a, dtype=np.float64), device="cuda")


def _vp(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def _padded(a, ld):
    """`a` in the top-left corner of a NaN-filled (ld, ld) buffer."""
    t = _nan(ld, ld)
    t[:a.shape[0], :a.shape[1]] = _dev(a)
    return t


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


class _Workspace:
    """`nbytes` of workspace followed by the guard band, all of it filled with a byte pattern."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        assert self.nbytes > 0
        self.buf = torch.full((self.nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        self.ptr = ctypes.c_void_p(self.buf.data_ptr())

    def doubles(self, byte_offset, count):
        return self.buf[byte_offset:byte_offset + 8 * count].view(torch.float64)

    def assert_guard_intact(self):
        torch.cuda.synchronize()
        assert bool((self.buf[self.nbytes:] == PATTERN).all()), "the kernels wrote past *_workspace_bytes"


def _rel_max(got, ref):
    """max |got - ref| over the largest |ref|, in the precision of the reference."""
    ref = np.asarray(ref)
    return float(np.abs(got.astype(ref.dtype) - ref).max() / np.abs(ref).max())


def _rel_each(got, ref):
    ref = np.asarray(ref)
    return float((np.abs(got.astype(ref.dtype) - ref) / np.abs(ref)).max())


def _over_terms(got, ref, mag):
    """max |got - ref| / sum |terms|, elementwise."""
    return float(_each_over_terms(got, ref, mag).max())


def _each_over_terms(got, ref, mag):
    ref = np.asarray(ref)
    diff = np.abs(got.astype(ref.dtype) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(diff == 0, 0, diff / mag)                            # no terms at all (n = 1: x_i - x_i): exactly 0 or inf


# ------------------------------------------------------------------------------------------------------------------ build_ky
@pytest.mark.parametrize("n,D", R.ladder())
def test_build_ky(G, n, D):
    pr = _problem(n, D)
    Kf_ref, Ky_ref = R.build(pr["X"], pr["lam"], pr["sf"], pr["noise"])
    X = _dev(pr["X"])
    _, lp = _lp(pr["lam"])
    Kf, Ky, Ky_alone = _nan(n, n), _nan(n, n), _nan(n, n)
    _check(_L().gpmpc_build_ky(n, D, _vp(X), lp, pr["sf"], pr["noise"], _vp(Kf), _vp(Ky), _sp()), "gpmpc_build_ky")
    _check(_L().gpmpc_build_ky(n, D, _vp(X), lp, pr["sf"], pr["noise"], None, _vp(Ky_alone), _sp()), "gpmpc_build_ky")
    torch.cuda.synchronize()
    e = max(_rel_each(Kf.cpu().numpy(), Kf_ref), _rel_each(Ky.cpu().numpy(), Ky_ref))
    print("  build_ky n %3d D %d: %.2e relative" % (n, D, e))
    assert _note("build_ky", e / TOL) <= 1
    assert _same_bits(Ky, Ky_alone)                                          # the Kf = NULL form writes the same Ky
    assert bool((torch.diagonal(Kf) == pr["sf"] * pr["sf"]).all())           # exp(0) = 1: sigma_f^2 exactly


# ------------------------------------------------------------------------------------------------------------------- predict
def _predict(pr, p, out_K=True, mean=True, cov=True, Xp=None):
    """One gpmpc_predict call on NaN-filled outputs and a guarded workspace; returns (K, mean, cov, W) as device tensors (K from the
    workspace when out_K is NULL)."""
    n, D = pr["n"], pr["D"]
    X, beta, Kinv = _dev(pr["X"]), _dev(pr["beta"]), _dev(pr["Kinv"])
    Xp = _dev(pr["Xp"][:p] if Xp is None else Xp)
    _, lp = _lp(pr["lam"])
    nb = _L().gpmpc_predict_workspace_bytes(n, D, p)
    ws = _Workspace(nb)
    K = _nan(p, n) if out_K else None
    m = _nan(p) if mean else None
    c = _nan(p, p) if cov else None
    _check(_L().gpmpc_predict(n, D, _vp(X), lp, pr["sf"], _vp(beta if mean else None), _vp(Kinv if cov else None), pr["noise"], p, _vp(Xp),
                              _vp(K), _vp(m), _vp(c), ws.ptr, ws.nbytes, _sp()), "gpmpc_predict")
    ws.assert_guard_intact()
    slab = (8 * p * n + 255) & ~255                                          # the layout of gpmpc_predict: [K | W | lambdas]
    assert nb == 2 * slab + 256
    if K is None:
        K = ws.doubles(0, p * n).reshape(p, n).clone()
    W = ws.doubles(slab, p * n).reshape(p, n).clone() if cov else None
    return K, m, c, W


@pytest.mark.parametrize("n,D", R.ladder())
def test_predict(G, n, D):
    pr = _problem(n, D)
    asym = np.abs(pr["Kinv"] - pr["Kinv"].T).max() / np.abs(pr["Kinv"]).max()
    for p in P_LADDER:
        ref = R.predict(pr["X"], pr["lam"], pr["sf"], pr["beta"], pr["Kinv"], pr["noise"], pr["Xp"][:p])
        K, m, c, W = _predict(pr, p)
        e_k = _rel_each(K.cpu().numpy(), ref["Ks"])
        e_m = _over_terms(m.cpu().numpy(), ref["mean"], ref["mean_abs"])
        e_w = _over_terms(W.cpu().numpy(), ref["W"], ref["W_abs"])
        e_c = _over_terms(c.cpu().numpy(), ref["cov"], ref["cov_abs"])
        print("  predict n %3d D %d p %2d: Ks %.2e  mean %.2e  W %.2e  cov %.2e (of the sum of |terms|)" % (n, D, p, e_k, e_m, e_w, e_c))
        assert _note("predict Ks", e_k / TOL) <= 1
        assert _note("predict mean", e_m / TOL) <= 1
        assert _note("predict W", e_w / TOL) <= 1
        assert _note("predict cov", e_c / TOL) <= 1
        if n >= 63 and p > 1:                                                # the inputs see K* K^-T: cov is not symmetric
            assert asym > 1e-4 and float((c - c.T).abs().max()) > 1e3 * TOL * float(ref["cov_abs"].max())
        # the output combinations agree bit for bit on what they share
        K2, m2, c2, W2 = _predict(pr, p, out_K=False)
        assert _same_bits(K, K2) and _same_bits(m, m2) and _same_bits(c, c2) and _same_bits(W, W2)
        K3, m3, _, _ = _predict(pr, p, cov=False)
        assert _same_bits(K, K3) and _same_bits(m, m3)
        K4, _, c4, W4 = _predict(pr, p, mean=False)
        assert _same_bits(K, K4) and _same_bits(c, c4) and _same_bits(W, W4)


@pytest.mark.parametrize("n,D", R.ladder())
def test_predict_rows_are_independent(G, n, D):
    """p = 9 points (a second row block of k_pred_w with seven padded rows) against the nine single-point calls (seven padded rows
    each, clamped to the one point): Ks, W, mean and the diagonal of cov bit for bit."""
    pr = _problem(n, D)
    K, m, c, W = _predict(pr, 9)
    for r in range(9):
        K1, m1, c1, W1 = _predict(pr, 1, Xp=pr["Xp"][r:r + 1])
        assert _same_bits(K[r], K1[0]) and _same_bits(W[r], W1[0]), r
        assert _same_bits(m[r:r + 1], m1) and _same_bits(c[r, r].reshape(1), c1.reshape(1)), r


# -------------------------------------------------------------------------------------------------------------------- matvec
@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 1000), (300, 7), (257, 257)])
def test_matvec(G, rows, cols):
    rng = np.random.default_rng(rows * 10007 + cols)
    A, v = rng.standard_normal((rows, cols)), rng.standard_normal(cols)
    ref, mag = R.dot_abs(R.cast(A), R.cast(v))
    out, Ad, vd = _nan(rows + 3), _dev(A), _dev(v)
    _check(_L().gpmpc_matvec(rows, cols, _vp(Ad), _vp(vd), _vp(out), _sp()), "gpmpc_matvec")
    torch.cuda.synchronize()
    e = _over_terms(out[:rows].cpu().numpy(), ref, mag)
    print("  matvec %d x %d: %.2e of the sum of |terms|" % (rows, cols, e))
    assert _note("matvec", e / TOL) <= 1
    assert bool(torch.isnan(out[rows:]).all())


# -------------------------------------------------------------------------------------------------------------------- append
def _kvec(pr):
    """K_f(X, x_new) rounded to float64: the k vector as data for gpmpc_kinv_append."""
    return R.to_f64(R.kernel(pr["X"], pr["xnew"][None, :], pr["lam"], pr["sf"]))[:, 0]


@pytest.mark.parametrize("n,D", R.ladder(schur=True))
def test_kinv_append(G, n, D):
    pr = _problem(n, D)
    k, kappa = _kvec(pr), pr["sf"] * pr["sf"] + pr["noise"]
    ref = R.append(pr["Kinv"], k, kappa)
    Kinv, kd = _dev(pr["Kinv"]), _dev(k)
    out = _nan(n + 2, n + 1)                                                 # one spare row: nothing may land behind the block
    ws = _Workspace(_L().gpmpc_kinv_append_workspace_bytes(n))
    _check(_L().gpmpc_kinv_append(n, _vp(Kinv), _vp(kd), kappa, _vp(out), ws.ptr, ws.nbytes, _sp()), "gpmpc_kinv_append")
    ws.assert_guard_intact()
    e = _rel_max(out[:n + 1].cpu().numpy(), ref)
    print("  kinv_append n %3d D %d: %.2e of the largest element" % (n, D, e))
    assert _note("kinv_append", e / TOL) <= 1
    assert bool(torch.isnan(out[n + 1]).all())
    assert np.array_equal(Kinv.cpu().numpy(), pr["Kinv"]) and np.array_equal(kd.cpu().numpy(), k)


@pytest.mark.parametrize("n,D", R.ladder(schur=True))
def test_gp_append(G, n, D):
    pr = _problem(n, D)
    ld_in, ld_out, m = n + 5, n + 12, n + 1
    sf, noise = pr["sf"], pr["noise"]
    kappa = sf * sf + noise
    X, xn = _dev(pr["X"]), _dev(pr["xnew"][None, :])
    _, lp = _lp(pr["lam"])
    src = [_padded(pr[name], ld_in) for name in ("Kf", "Ky", "Kinv")]
    src_copy = [t.clone() for t in src]
    out = [_nan(ld_out, ld_out) for _ in range(3)]
    ws = _Workspace(_L().gpmpc_gp_append_workspace_bytes(n, D))
    _check(_L().gpmpc_gp_append(n, D, _vp(X), _vp(xn), lp, sf, noise, _vp(src[0]), _vp(src[1]), ld_in, _vp(src[2]), ld_in,
                                _vp(out[0]), _vp(out[1]), _vp(out[2]), ld_out, ws.ptr, ws.nbytes, _sp()), "gpmpc_gp_append")
    ws.assert_guard_intact()
    for a, b in zip(src, src_copy):                                          # inputs untouched, NaN padding included
        assert _same_bits(a, b)
    for t in out:                                                            # nothing outside the (n + 1)^2 block
        assert bool(torch.isnan(t[m:, :]).all()) and bool(torch.isnan(t[:, m:]).all()) and not bool(torch.isnan(t[:m, :m]).any())
    Xall = np.concatenate((pr["X"], pr["xnew"][None, :]))
    Kf_ref, Ky_ref = R.build(Xall, pr["lam"], sf, noise)
    e_k = max(_rel_each(out[0][:m, :m].cpu().numpy(), Kf_ref), _rel_each(out[1][:m, :m].cpu().numpy(), Ky_ref))
    ref = R.append(pr["Kinv"], R.kernel(pr["X"], pr["xnew"][None, :], pr["lam"], sf)[:, 0], R.cast(sf) * R.cast(sf) + R.cast(noise))
    e = _rel_max(out[2][:m, :m].cpu().numpy(), ref)
    print("  gp_append n %3d D %d: Ky_inv %.2e of the largest element, Kf / Ky %.2e relative" % (n, D, e, e_k))
    assert _note("gp_append Kf Ky", e_k / TOL) <= 1
    assert _note("gp_append", e / TOL) <= 1
    # "Same expressions, same summation orders": gpmpc_predict for k, then gpmpc_kinv_append, gives the same bits
    kd, _, _, _ = _predict(pr, 1, mean=False, cov=False, Xp=pr["xnew"][None, :])
    two, Kinv = _nan(m, m), _dev(pr["Kinv"])
    ws2 = _Workspace(_L().gpmpc_kinv_append_workspace_bytes(n))
    _check(_L().gpmpc_kinv_append(n, _vp(Kinv), _vp(kd), kappa, _vp(two), ws2.ptr, ws2.nbytes, _sp()), "gpmpc_kinv_append")
    ws2.assert_guard_intact()
    assert _same_bits(out[0][:n, n], kd[0]) and _same_bits(out[2][:m, :m], two)


# -------------------------------------------------------------------------------------------------------------------- remove
@pytest.mark.parametrize("n,D", [c for c in R.ladder(schur=True) if c[0] >= 2])
def test_kinv_remove(G, n, D):
    pr = _problem(n, D)
    ld_in, ld_out, m = n + 5, n + 3, n - 1
    src = _padded(pr["Kinv"], ld_in)
    src_copy = src.clone()
    for p in R.slots(n):
        out = _nan(ld_out, ld_out)
        _check(_L().gpmpc_kinv_remove(n, _vp(src), ld_in, p, _vp(out), ld_out, _sp()), "gpmpc_kinv_remove")
        torch.cuda.synchronize()
        e = _rel_max(out[:m, :m].cpu().numpy(), R.remove(pr["Kinv"], p))
        print("  kinv_remove n %3d D %d index %3d: %.2e of the largest element" % (n, D, p, e))
        assert _note("kinv_remove", e / TOL) <= 1
        assert bool(torch.isnan(out[m:, :]).all()) and bool(torch.isnan(out[:, m:]).all())
    assert _same_bits(src, src_copy)


# ------------------------------------------------------------------------------------------------------------------- replace
@pytest.mark.parametrize("n,D", R.ladder(schur=True))
def test_gp_replace(G, n, D):
    pr = _problem(n, D)
    ld_in, ld_out = n + 5, n + 12
    sf, noise = pr["sf"], pr["noise"]
    X, xn = _dev(pr["X"]), _dev(pr["xnew"][None, :])
    _, lp = _lp(pr["lam"])
    src = [_padded(pr[name], ld_in) for name in ("Kf", "Ky", "Kinv")]
    src_copy = [t.clone() for t in src]
    kt_ref = R.kernel(pr["X"], pr["xnew"][None, :], pr["lam"], sf)[:, 0]
    kappa_ref = R.cast(sf) * R.cast(sf) + R.cast(noise)
    for p in R.slots(n):
        outs = []
        for rep in range(2):
            out = [_nan(ld_out, ld_out) for _ in range(3)]
            ws = _Workspace(_L().gpmpc_gp_replace_workspace_bytes(n, D))
            _check(_L().gpmpc_gp_replace(n, D, p, _vp(X), _vp(xn), lp, sf, noise, _vp(src[0]), _vp(src[1]), ld_in, _vp(src[2]), ld_in,
                                         _vp(out[0]), _vp(out[1]), _vp(out[2]), ld_out, ws.ptr, ws.nbytes, _sp()), "gpmpc_gp_replace")
            ws.assert_guard_intact()
            outs.append(out)
        for a, b in zip(*outs):                                              # fixed summation order: two calls, the same bits
            assert _same_bits(a, b)
        out = outs[0]
        for t in out:
            assert bool(torch.isnan(t[n:, :]).all()) and bool(torch.isnan(t[:, n:]).all()) and not bool(torch.isnan(t[:n, :n]).any())
        v, w = ws.doubles(0, n), ws.doubles(8 * n, n)                        # workspace: [v | w | kt]
        assert float(v[p]) == 0.0 and float(w[p]) == 0.0 and float(ws.doubles(16 * n, n)[p]) == 0.0
        X_new = np.array(pr["X"])
        X_new[p] = pr["xnew"]
        Kf_ref, Ky_ref = R.build(X_new, pr["lam"], sf, noise)
        e_k = max(_rel_each(out[0][:n, :n].cpu().numpy(), Kf_ref), _rel_each(out[1][:n, :n].cpu().numpy(), Ky_ref))
        e = _rel_max(out[2][:n, :n].cpu().numpy(), R.replace(pr["Kinv"], kt_ref, kappa_ref, p))
        print("  gp_replace n %3d D %d slot %3d: Ky_inv %.2e of the largest element, Kf / Ky %.2e relative" % (n, D, p, e, e_k))
        assert _note("gp_replace Kf Ky", e_k / TOL) <= 1
        assert _note("gp_replace", e / TOL) <= 1
    for a, b in zip(src, src_copy):
        assert _same_bits(a, b)


# ------------------------------------------------------------------------------------------------------------------- ml_grad
@pytest.mark.parametrize("n,D", R.ladder())
def test_ml_grad(G, n, D):
    pr = _problem(n, D)
    alpha, resid = pr["beta"], pr["y"]                                       # alpha = Ky_inv r in float64: data to the kernel
    val, mag = R.ml_grad(pr["X"], pr["Kinv"], alpha, resid, pr["lam"], pr["sf"], pr["noise"])
    X, Kinv, a, r = _dev(pr["X"]), _dev(pr["Kinv"]), _dev(alpha), _dev(resid)
    _, lp = _lp(pr["lam"])
    outs = []
    for rep in range(2):
        out = _nan(D + 4)
        ws = _Workspace(_L().gpmpc_ml_grad_workspace_bytes(n, D))
        _check(_L().gpmpc_ml_grad(n, D, _vp(X), _vp(Kinv), _vp(a), _vp(r), lp, pr["sf"], pr["noise"], _vp(out), ws.ptr, ws.nbytes, _sp()),
               "gpmpc_ml_grad")
        ws.assert_guard_intact()
        outs.append(out)
    assert _same_bits(outs[0][:D + 3], outs[1][:D + 3]) and bool(torch.isnan(outs[0][D + 3]))
    e = _each_over_terms(outs[0][:D + 3].cpu().numpy(), val, mag)
    print("  ml_grad n %3d D %d: lambda %.2e  sigma_f %.2e  sigma_n %.2e  r.alpha %.2e (of the sum of |terms|)"
          % (n, D, float(e[:D].max()), float(e[D]), float(e[D + 1]), float(e[D + 2])))
    assert _note("ml_grad", float(e.max()) / TOL) <= 1


# ----------------------------------------------------------------------------------------------------------------- workspace
def test_one_byte_less_of_workspace_is_refused_before_anything_is_launched(G):
    n, D, p = 65, 2, 9
    pr = _problem(n, D)
    L = _L()
    X, xn, Xp, Kinv, beta, y = (_dev(a) for a in (pr["X"], pr["xnew"][None, :], pr["Xp"][:p], pr["Kinv"], pr["beta"], pr["y"]))
    _, lp = _lp(pr["lam"])
    src = [_dev(pr[name]) for name in ("Kf", "Ky", "Kinv")]
    sf, noise = pr["sf"], pr["noise"]

    def refused(nbytes, call, outs):
        ws = _Workspace(nbytes)
        assert call(ws.ptr, nbytes - 1) == E_WORKSPACE
        torch.cuda.synchronize()
        assert bool((ws.buf == PATTERN).all())                               # not even the workspace was touched
        for t in outs:
            assert bool(torch.isnan(t).all())

    K, m, c = _nan(p, n), _nan(p), _nan(p, p)
    refused(L.gpmpc_predict_workspace_bytes(n, D, p),
            lambda w, nb: L.gpmpc_predict(n, D, _vp(X), lp, sf, _vp(beta), _vp(Kinv), noise, p, _vp(Xp), _vp(K), _vp(m), _vp(c), w, nb, _sp()),
            (K, m, c))
    o = _nan(n + 1, n + 1)
    refused(L.gpmpc_kinv_append_workspace_bytes(n),
            lambda w, nb: L.gpmpc_kinv_append(n, _vp(Kinv), _vp(beta), 1.5, _vp(o), w, nb, _sp()), (o,))
    out = [_nan(n + 1, n + 1) for _ in range(3)]
    refused(L.gpmpc_gp_append_workspace_bytes(n, D),
            lambda w, nb: L.gpmpc_gp_append(n, D, _vp(X), _vp(xn), lp, sf, noise, _vp(src[0]), _vp(src[1]), n, _vp(src[2]), n,
                                            _vp(out[0]), _vp(out[1]), _vp(out[2]), n + 1, w, nb, _sp()), out)
    refused(L.gpmpc_gp_replace_workspace_bytes(n, D),
            lambda w, nb: L.gpmpc_gp_replace(n, D, 3, _vp(X), _vp(xn), lp, sf, noise, _vp(src[0]), _vp(src[1]), n, _vp(src[2]), n,
                                             _vp(out[0]), _vp(out[1]), _vp(out[2]), n + 1, w, nb, _sp()), out)
    g = _nan(D + 3)
    refused(L.gpmpc_ml_grad_workspace_bytes(n, D),
            lambda w, nb: L.gpmpc_ml_grad(n, D, _vp(X), _vp(Kinv), _vp(beta), _vp(y), lp, sf, noise, _vp(g), w, nb, _sp()), (g,))


# ------------------------------------------------------------------------------------------------------------------- classes
def test_classes_replace_and_remove_across_the_256_column_block(G):
    """GaussianProcessRegression with 300 points: the O(N^2) replacement at slots 0, 255, 256, 299 and the removal of 256 against a
    from-scratch GP on the same rows (1e-9 of the largest element: the tolerance of the append's ABI test against a fresh inverse)."""
    rng = np.random.default_rng(300)
    n, D = 300, 3
    X = rng.uniform(-2, 2, (n + 4, D))
    y = np.sin(X).sum(axis=1)

    def gp_on(Xr, yr):
        g = G.GaussianProcessRegression(D)
        g.set_lambdas(np.array([0.9, 1.6, 2.2])); g.set_sigma_f(np.array(1.2)); g.set_sigma_n(np.array(0.36))
        g.append_train_data(Xr, yr)
        return g

    def against_scratch(what):
        ref = gp_on(Xw, yw)
        assert torch.equal(inc.X_train, ref.X_train) and torch.equal(inc.y_train, ref.y_train)
        np.testing.assert_allclose(inc.Kf.cpu().numpy(), ref.Kf.cpu().numpy(), rtol=1e-13, atol=0)
        np.testing.assert_allclose(inc.Ky.cpu().numpy(), ref.Ky.cpu().numpy(), rtol=1e-13, atol=0)
        err = float((inc.Ky_inv - ref.Ky_inv).abs().max()) / float(ref.Ky_inv.abs().max())
        print("  %s: Ky_inv %.2e of the largest element against a from-scratch GP" % (what, err))
        assert _note("classes", err / 1e-9) <= 1

    Xw, yw = X[:n].copy(), y[:n].copy()
    inc = gp_on(Xw, yw)
    for j, slot in enumerate((0, 255, 256, 299)):
        inc.replace_train_data(slot, X[n + j], float(y[n + j]), incremental=True)
        Xw[slot], yw[slot] = X[n + j], y[n + j]
        assert inc._appends_since_rebuild == j + 1 and inc.num_train == n     # the O(N^2) path, not a rebuild
        against_scratch("replace slot %3d" % slot)
    inc.remove_train_data(256, incremental=True)
    Xw, yw = np.delete(Xw, 256, axis=0), np.delete(yw, 256)
    assert inc._appends_since_rebuild == 5 and inc.num_train == n - 1
    against_scratch("remove 256")
