"""The sparse GP (FITC inducing points) on the device against tests/sparse_reference.py.

Kernel level (gpmpc_sparse_accumulate / _finish / _append): a ladder of sizes that puts one point either side of every stage and tile
edge of the kernels, padded row strides in NaN-filled buffers, outputs pre-filled with NaN, workspaces of exactly *_workspace_bytes
followed by a guard band.  Tolerance rule, per case and output array: with e64 the max-abs error of the reference's float64 evaluation
against its extended-precision one on the same inputs, the device is allowed max(8 e64, 1e-13 max|array|)  (sparse_reference.allowance).
The bit-for-bit properties the header promises are asserted as such.

End to end (SparseDynamics -> pack -> rollout) at the project's figures -- means rtol 1e-5, variances and gradient rtol 1e-4, cost rtol
1e-6, the small atol of smoke() -- against the reference rollout built from the pinned oracle's own pieces; tests/test_host_sparse.py
holds the float64 restatement ten-fold under each of them and shows that three deliberate mistakes exceed them a hundred-fold.

Worst error / allowance per entry point as printed by a run on an MI355X: see DESIGN.md section 3h."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sparse_reference as R
from test_host_sparse import E2E_TOL, e2e_problem

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 4096, 0xA5
E_WORKSPACE = -4
_WORST = {}


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    yield g
    print("\n  worst error / allowance per entry point: " + ", ".join("%s %.3f" % kv for kv in sorted(_WORST.items())))


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
    """`a` [rows][cols] in the left columns of a NaN-filled [rows][ld] buffer."""
    a = np.asarray(a)
    t = _nan(a.shape[0], ld)
    t[:, :a.shape[1]] = _dev(a)
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

    def assert_guard_intact(self):
        torch.cuda.synchronize()
        assert bool((self.buf[self.nbytes:] == PATTERN).all()), "the kernels wrote past *_workspace_bytes"


@functools.lru_cache(maxsize=None)
def _problem(M, n, D, nt):
    return R.problem(R.seed_of(M, n, D, nt), n, M, D, nt)


@functools.lru_cache(maxsize=None)
def _reference(M, n, D, nt):
    """Extended-precision and float64 evaluations of accumulate / finish / append on the float64 inputs of the case (computed once)."""
    pr = _problem(M, n, D, nt)
    hyp = (pr["lam"], pr["sf"], pr["noise"])
    acc_ld = R.accumulate(pr["X"], pr["Y"], pr["Z"], pr["W"], *hyp)
    # finish and append start from float64 data: G, r and Q rounded from the extended-precision evaluation (Q symmetric), and Binv
    G64, r64 = R.to_f64(acc_ld["G"]), R.to_f64(acc_ld["r"])
    G64 = (G64 + G64.T) / 2
    Q64 = R.to_f64(R.finish(pr["W"], pr["Binv"], r64)["Q"])
    Q64 = (Q64 + Q64.T) / 2
    out = {"G64": G64, "r64": r64, "Q64": Q64}
    for tag, prec in (("ld", None), ("f64", np.float64)):
        out[tag] = {"acc": acc_ld if prec is None else R.accumulate(pr["X"], pr["Y"], pr["Z"], pr["W"], *hyp, prec=prec),
                    "fin": R.finish(pr["W"], pr["Binv"], r64, prec=prec),
                    "app": R.append(pr["xnew"], pr["ynew"], pr["Z"], pr["W"], *hyp, G64, r64, pr["Binv"], Q64, prec=prec)}
    return out


def _hold(name, got, ref, key_path, label):
    ld, f64 = ref["ld"], ref["f64"]
    for k in key_path:
        ld, f64 = ld[k], f64[k]
    allow = R.allowance(ld, f64)
    e = R.err(got, ld)
    ratio = e / allow
    print("  %-28s %-6s err %.2e allowance %.2e (%.3f)" % (label, key_path[-1], e, allow, ratio))
    assert _note(name, ratio) <= 1, (label, key_path, e, allow)


def _accumulate(pr, chunk, accumulate=0, rows=None, ld_w=None, ld_y=None, out=None, nt=None, Y=None):
    """One gpmpc_sparse_accumulate call on rows [rows[0], rows[1]) with padded strides; returns (G, r, stats) device tensors."""
    M, D = pr["M"], pr["D"]
    Yh = pr["Y"] if Y is None else Y
    nt = Yh.shape[1] if nt is None else nt
    lo, hi = (0, pr["n"]) if rows is None else rows
    ld_w, ld_y = ld_w or M + 3, ld_y or Yh.shape[1] + 2
    X, Yd, Z, W = _dev(pr["X"][lo:hi]), _padded(Yh[lo:hi], ld_y), _dev(pr["Z"]), _padded(pr["W"], ld_w)
    Gd, rd, st = out if out is not None else (_nan(M, M), _nan(M, nt), _nan(2))
    nb = _L().gpmpc_sparse_accumulate_workspace_bytes(hi - lo, D, M, nt, chunk)
    ws = _Workspace(nb)
    args = (hi - lo, D, M, nt, _vp(X), _vp(Yd), ld_y, _vp(Z), _vp(W), ld_w, _lp(pr["lam"])[1], pr["sf"], pr["noise"], chunk, accumulate,
            _vp(Gd), _vp(rd), _vp(st), ws.ptr)
    assert _L().gpmpc_sparse_accumulate(*args, nb - 1, _sp()) == E_WORKSPACE
    _check(_L().gpmpc_sparse_accumulate(*args, nb, _sp()), "gpmpc_sparse_accumulate")
    ws.assert_guard_intact()
    return Gd, rd, st


FORMS = {"fma": 0, "mfma": 1}


@pytest.fixture(params=sorted(FORMS))
def form(request, G):
    """Both forms of the two N M^2 products (gpmpc_sparse_set_form), the process-wide choice restored afterwards."""
    old = _L().gpmpc_sparse_set_form(FORMS[request.param])
    assert old in (0, 1)
    yield request.param
    assert _L().gpmpc_sparse_set_form(old) == FORMS[request.param]


def test_set_form(G):
    L = _L()
    cur = L.gpmpc_sparse_set_form(-1)
    assert cur in (0, 1)                                                     # GPMPC_SPARSE_FORM_DEFAULT: the measured choice
    other = 1 - cur
    assert L.gpmpc_sparse_set_form(other) == cur and L.gpmpc_sparse_set_form(-1) == other
    assert L.gpmpc_sparse_set_form(2) == -1 and "gpmpc_sparse_set_form" in L.gpmpc_last_error().decode() and L.gpmpc_sparse_set_form(-1) == other
    assert L.gpmpc_sparse_set_form(cur) == other
    # the two forms agree to rounding (not bit for bit: another summation order)
    pr = _problem(130, 200, 8, 4)
    Ga, ra, sa = _accumulate(pr, 64)
    L.gpmpc_sparse_set_form(other)
    try:
        Gb, rb, sb = _accumulate(pr, 64)
    finally:
        L.gpmpc_sparse_set_form(cur)
    assert float((Ga - Gb).abs().max()) <= 1e-11 * float(Ga.abs().max()) and float((ra - rb).abs().max()) <= 1e-11 * float(ra.abs().max())
    assert not _same_bits(Ga, Gb) and sa[0].item() == sb[0].item()


# ------------------------------------------------------------------------------------------------------------------ kernel ladder
@pytest.mark.parametrize("M,n,D,nt", R.ladder())
def test_accumulate_finish_append_ladder(G, form, M, n, D, nt):
    pr, ref = _problem(M, n, D, nt), _reference(M, n, D, nt)
    label = "%-4s M %3d n %3d D %d nt %d" % (form, M, n, D, nt)
    for chunk in (0, 64):
        Gd, rd, st = _accumulate(pr, chunk)
        tag = label + " chunk %d" % chunk
        _hold("accumulate_" + form, Gd.cpu().numpy(), ref, ("acc", "G"), tag)
        _hold("accumulate_" + form, rd.cpu().numpy(), ref, ("acc", "r"), tag)
        _hold("accumulate_" + form, st[1:].cpu().numpy(), ref, ("acc", "min_lambda"), tag)
        assert st[0].item() == n
        assert _same_bits(Gd, Gd.T)
    if form != "fma":                                                        # finish and append have one form
        return
    # finish: alpha, Q from (W, Binv, r) -- float64 data
    ld_w = M + 5
    W, Binv, r = _padded(pr["W"], ld_w), _dev(pr["Binv"]), _dev(ref["r64"])
    alpha, Q = _nan(M, nt), _nan(M, M)
    nb = _L().gpmpc_sparse_finish_workspace_bytes(M, nt)
    ws = _Workspace(nb)
    args = (M, nt, _vp(W), ld_w, _vp(Binv), _vp(r), _vp(alpha), _vp(Q), ws.ptr)
    assert _L().gpmpc_sparse_finish(*args, nb - 1, _sp()) == E_WORKSPACE
    _check(_L().gpmpc_sparse_finish(*args, nb, _sp()), "gpmpc_sparse_finish")
    ws.assert_guard_intact()
    _hold("finish", alpha.cpu().numpy(), ref, ("fin", "alpha"), label)
    _hold("finish", Q.cpu().numpy(), ref, ("fin", "Q"), label)
    assert _same_bits(Q, Q.T)
    # append: one observation onto the float64 state (G64, r64, Binv, Q64)
    Gd, rd, Bd, Qd, ad = _dev(ref["G64"]), _dev(ref["r64"]), _dev(pr["Binv"]), _dev(ref["Q64"]), _nan(M, nt)
    st = _dev([float(n), 7.0])
    x, y, Z = _dev(pr["xnew"]), _dev(pr["ynew"]), _dev(pr["Z"])
    nb = _L().gpmpc_sparse_append_workspace_bytes(M, nt)
    ws = _Workspace(nb)
    args = (D, M, nt, _vp(x), _vp(y), _vp(Z), _vp(W), ld_w, _lp(pr["lam"])[1], pr["sf"], pr["noise"], _vp(Gd), _vp(rd), _vp(Bd), _vp(Qd),
            _vp(ad), _vp(st), ws.ptr)
    assert _L().gpmpc_sparse_append(*args, nb - 1, _sp()) == E_WORKSPACE
    _check(_L().gpmpc_sparse_append(*args, nb, _sp()), "gpmpc_sparse_append")
    ws.assert_guard_intact()
    for k, t in (("G", Gd), ("r", rd), ("Binv", Bd), ("Q", Qd), ("alpha", ad)):
        _hold("append", t.cpu().numpy(), ref, ("app", k), label)
    _hold("append", st[1:].cpu().numpy(), ref, ("app", "Lambda"), label)      # (7.0 is above every Lambda here: the minimum is the new one)
    assert st[0].item() == n + 1
    assert _same_bits(Gd, Gd.T) and _same_bits(Bd, Bd.T) and _same_bits(Qd, Qd.T)


# ------------------------------------------------------------------------------------------------------------------ bit-for-bit properties
@pytest.mark.parametrize("M,n,D", [(33, 200, 5), (130, 200, 2), (16, 65, 8)])
def test_accumulate_bit_properties(G, form, M, n, D):
    pr = _problem(M, n, D, 4)
    chunk = 64
    G1, r1, s1 = _accumulate(pr, chunk)
    G2, r2, s2 = _accumulate(pr, chunk, ld_w=M + 11, ld_y=9)
    assert _same_bits(G1, G2) and _same_bits(r1, r2) and _same_bits(s1, s2)              # identical calls (and strides do not matter)
    assert _same_bits(G1, G1.T)
    # G does not depend on n_targets; column a of r does not depend on the other columns
    Gn, rn, _ = _accumulate(pr, chunk, nt=1)
    assert _same_bits(Gn, G1) and _same_bits(rn[:, 0], r1[:, 0])
    Y2 = np.array(pr["Y"])
    Y2[:, (0, 1, 3)] = np.random.default_rng(1).standard_normal((n, 3)) * 1e3
    _, r3, _ = _accumulate(pr, chunk, Y=Y2)
    assert _same_bits(r3[:, 2], r1[:, 2]) and not _same_bits(r3[:, 1], r1[:, 1])
    # rows [0, n) in one call == rows [0, s) then accumulate = 1 over [s, n), s a multiple of chunk
    for s in (64, 128):
        if s >= n:
            continue
        out = _accumulate(pr, chunk, rows=(0, s))
        Gs, rs, ss = _accumulate(pr, chunk, accumulate=1, rows=(s, n), out=out)
        assert _same_bits(Gs, G1) and _same_bits(rs, r1) and _same_bits(ss, s1)
    # the result may depend on chunk -- to rounding only
    G0, r0, s0 = _accumulate(pr, 0)
    assert float((G0 - G1).abs().max()) <= 1e-12 * float(G1.abs().max()) and s0[0].item() == s1[0].item() == n


def test_refusals_with_device_buffers(G):
    pr = _problem(16, 65, 8, 4)
    Gd, rd, st = _accumulate(pr, 64)
    before = Gd.clone()
    M, D, nt = 16, 8, 4
    X, Y, Z, W = _dev(pr["X"]), _dev(pr["Y"]), _dev(pr["Z"]), _dev(pr["W"])
    ws = _Workspace(_L().gpmpc_sparse_accumulate_workspace_bytes(65, D, M, nt, 64))
    for kw in (dict(n=0), dict(M=0), dict(chunk=65), dict(ld_y=3), dict(ld_w=15), dict(nt=9), dict(D=9)):
        a = dict(n=65, D=D, M=M, nt=nt, ld_y=4, ld_w=16, chunk=64)
        a.update(kw)
        rc = _L().gpmpc_sparse_accumulate(a["n"], a["D"], a["M"], a["nt"], _vp(X), _vp(Y), a["ld_y"], _vp(Z), _vp(W), a["ld_w"], _lp(pr["lam"])[1],
                                          pr["sf"], pr["noise"], a["chunk"], 1, _vp(Gd), _vp(rd), _vp(st), ws.ptr, ws.nbytes, _sp())
        assert rc == -1 and _L().gpmpc_last_error().decode().startswith("gpmpc_sparse_accumulate"), kw
    torch.cuda.synchronize()
    assert _same_bits(Gd, before)                                            # refused before any launch


# ------------------------------------------------------------------------------------------------------------------ SparseGPState
@functools.lru_cache(maxsize=None)
def _e2e(tag):
    return e2e_problem(tag)


def test_260_appends_equal_the_batch_fit(G):
    """40 rows fitted, 260 single appends (default refresh_every = 64: four refreshes on the way), against ONE batch fit of all 300 rows,
    under the same allowance rule; the W the state built is data for the reference."""
    pb, Z = _e2e("ds2")
    lam, sf, sn = pb["lambdas"][0], 1.0, 1e-2
    st = G.SparseGPState(Z, lam, sf, sn)
    assert st.refresh_every == 64
    X, Y = _dev(pb["X"]), _dev(pb["Y"][:, :1])
    st.fit(X[:40], Y[:40])
    assert st.num_obs == 40
    for i in range(40, 300):
        st.append(X[i], Y[i])
    assert st._appends == 260 % 64                                           # the last four observations went in by the rank-one formulas alone
    assert st.num_obs == 300 and _same_bits(st.Q, st.Q.T) and _same_bits(st.G, st.G.T) and _same_bits(st.Binv, st.Binv.T)
    W = st.W.cpu().numpy()
    ld = R.fit(pb["X"], pb["Y"][:, :1], Z, lam, sf, sn * sn, st.jitter, W=W)
    f64 = R.fit(pb["X"], pb["Y"][:, :1], Z, lam, sf, sn * sn, st.jitter, W=W, prec=np.float64)
    for k in ("G", "r", "alpha", "Q"):
        allow, e = R.allowance(ld[k], f64[k]), R.err(getattr(st, k).cpu().numpy(), ld[k])
        print("  260 appends against the batch fit, %-5s err %.2e allowance %.2e (%.3f)" % (k, e, allow, e / allow))
        assert _note("appends_vs_batch", e / allow) <= 1, k
    allow = R.allowance(np.array([ld["min_lambda"]]), np.array([f64["min_lambda"]]))
    assert R.err(np.array([st.min_lambda]), np.array([ld["min_lambda"]])) <= allow
    # ... and against the state's own batch fit of the same rows (another route to the same numbers: both within the allowance of the reference)
    st2 = G.SparseGPState(Z, lam, sf, sn).fit(X, Y)
    assert R.err(st2.alpha.cpu().numpy(), ld["alpha"]) <= R.allowance(ld["alpha"], f64["alpha"])
    # predict goes through gpmpc_predict with (Z, alpha, Q)
    Xs = pb["X"][:7] + 0.05
    mean, cov = st2.predict(Xs)
    m_ref, v_ref = R.predict(Z, R.to_f64(ld["alpha"]), R.to_f64(ld["Q"]), lam, sf, Xs)
    np.testing.assert_allclose(mean.cpu().numpy(), R.to_f64(m_ref), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(torch.diagonal(cov).cpu().numpy(), R.to_f64(v_ref), rtol=1e-6, atol=1e-12)


def test_state_raises_on_nonpositive_lambda(G):
    """sigma_n = 0 and jitter = 0 with Z = X: Lambda_n = sigma_f^2 - |v_n|^2 is zero up to rounding, negative for some n."""
    pb, _ = _e2e("ds2")
    X = pb["X"][:40]
    st = G.SparseGPState(X, pb["lambdas"][0] / 20, 1.0, 0.0, jitter=0.0)
    with pytest.raises(FloatingPointError, match="Lambda"):
        st.fit(X, pb["Y"][:40, :1])


# ------------------------------------------------------------------------------------------------------------------ end to end
def _sparse_dynamics(G, pb, Z, **kw):
    dyn = G.SparseDynamics(pb["ds"], pb["da"], Z, **kw)
    for a, g in enumerate(dyn.gpr_err):
        g.set_lambdas(pb["lambdas"][a])
        g.set_sigma_n(float(pb["sigma_n"][a]))
        g.set_sigma_f(1.0)
    dyn.append_train_data(pb["X"][:, :pb["ds"]], pb["X"][:, pb["ds"]:], pb["Y"])
    return dyn


def _effective(pb, dyn):
    """The problem with the hyper-parameters as the GP objects hold them (set through log / exp; float32 noise variance): data to the reference."""
    return dict(pb, lambdas=np.stack([g.get_lambdas() for g in dyn.gpr_err]), sigma_f=np.array([g.get_sigma_f() for g in dyn.gpr_err]),
                sigma_n=np.sqrt(np.array([g._noise_var() for g in dyn.gpr_err])))


@functools.lru_cache(maxsize=None)
def _e2e_setup(tag):
    import gaussian_process_mpc_amd as g
    pb, Z = _e2e(tag)
    dyn = _sparse_dynamics(g, pb, Z)
    pe = _effective(pb, dyn)
    alpha, Q = R.fit_bundle(pe, Z)
    return pb, pe, Z, dyn, alpha, Q


@functools.lru_cache(maxsize=None)
def _e2e_ref(tag, b, fullcov=False):
    pb, pe, Z, dyn, alpha, Q = _e2e_setup(tag)
    return R.rollout(Z, alpha, Q, pe["lambdas"], pe["sigma_f"], pb["H"], pb["x0"][b], pb["U"][b], pb["Q"], pb["R"], -1.0, fullcov=fullcov)


def _assert_e2e(got, ref, keys, label):
    for k in keys:
        rtol, atol = E2E_TOL[k]
        g, r = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        ratio = float(np.max(np.abs(g - r) / (atol + rtol * np.abs(r))))
        print("  %-34s %-5s %.3g of its tolerance" % (label, k, ratio))
        _note("e2e_" + k, ratio)
        np.testing.assert_allclose(g, r, rtol=rtol, atol=atol, err_msg="%s %s" % (label, k))


@pytest.mark.parametrize("tag", ["ds2", "ds4"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("want_grad", [True, False], ids=["grad", "nograd"])
def test_end_to_end_rollout(G, tag, B, want_grad):
    pb, pe, Z, dyn, alpha, Q = _e2e_setup(tag)
    a_dev, Q_dev = dyn.posterior()
    assert a_dev.shape == (Z.shape[0], pb["ds"])
    cost = G.CostParams(-1.0, pb["Q"], pb["R"])
    r = dyn.rollout(pb["x0"][:B], pb["U"][:B], cost, want_grad=want_grad)
    torch.cuda.synchronize()
    assert ("grad" in r) == want_grad and dyn.pack().N == Z.shape[0]
    for b in range(B):
        got = {k: v[b].cpu().numpy() for k, v in r.items()}
        _assert_e2e(got, _e2e_ref(tag, b), ("means", "vars", "cost") + (("grad",) if want_grad else ()), "%s B %d traj %d" % (tag, B, b))


@pytest.mark.parametrize("tag", ["ds2", "ds4"])
def test_end_to_end_autograd(G, tag):
    """The reference's pattern forward_propagate_torch -> cost_torch -> backward() on a controller whose dynamics are sparse."""
    pb, pe, Z, dyn, alpha, Q = _e2e_setup(tag)
    H, ds, da = pb["H"], pb["ds"], pb["da"]
    mpc = G.RiskSensitiveMPC(-1.0, H, ds, da, pb["Q"], pb["R"])
    mpc.dynamics = dyn
    u = torch.as_tensor(pb["U"][0], device=mpc.device).type(torch.float64).requires_grad_(True)
    means, covs = dyn.forward_propagate_torch(H, torch.as_tensor(pb["x0"][0], device=mpc.device), u)
    c = mpc.cost_torch(means, u, covs, mpc.x_ref, mpc.u_ref)
    c.backward()
    got = {"means": torch.stack(means).detach().cpu().numpy(), "vars": torch.stack([torch.diagonal(s) for s in covs]).detach().cpu().numpy(),
           "cost": c.item(), "grad": u.grad.cpu().numpy()}
    _assert_e2e(got, _e2e_ref(tag, 0), ("means", "vars", "cost", "grad"), "%s autograd" % tag)
    m_np, c_np = dyn.forward_propagate(H, pb["x0"][0], pb["U"][0])
    np.testing.assert_allclose(m_np, got["means"], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("tag", ["ds2", "ds4"])
def test_end_to_end_full_covariance(G, tag):
    pb, pe, Z, dyn, alpha, Q = _e2e_setup(tag)
    cost = G.CostParams(-1.0, pb["Q"], pb["R"])
    r = dyn.rollout(pb["x0"], pb["U"], cost, want_grad=True, full_covariance=True)
    torch.cuda.synchronize()
    for b in range(pb["B"]):
        got = {k: v[b].cpu().numpy() for k, v in r.items()}
        _assert_e2e(got, _e2e_ref(tag, b, True), ("means", "covs", "cost", "grad"), "%s fullcov traj %d" % (tag, b))


# ------------------------------------------------------------------------------------------------------------------ behaviour
def test_inducing_at_the_data_is_the_dense_dynamics(G):
    """SparseDynamics with Z = X and jitter = 0 against Dynamics on the N = 40 problem: the same rollout."""
    from gaussian_process_mpc_amd.synth import synth_problem
    pb = synth_problem(7, 40, 2, 1, 5, 2, lam_range=(0.3, 0.6))
    sp = _sparse_dynamics(G, pb, pb["X"], jitter=0.0)
    de = G.Dynamics(2, 1)
    for a, g in enumerate(de.gpr_err):
        g.set_lambdas(pb["lambdas"][a])
        g.set_sigma_n(float(pb["sigma_n"][a]))
        g.set_sigma_f(1.0)
    de.append_train_data(pb["X"][:, :2], pb["X"][:, 2:], pb["Y"])
    cost = G.CostParams(-1.0, pb["Q"], pb["R"])
    rs, rd = sp.rollout(pb["x0"], pb["U"], cost, want_grad=True), de.rollout(pb["x0"], pb["U"], cost, want_grad=True)
    for k in ("means", "vars", "cost", "grad"):
        rtol, atol = E2E_TOL[k]
        np.testing.assert_allclose(rs[k].cpu().numpy(), rd[k].cpu().numpy(), rtol=rtol, atol=atol, err_msg=k)
    assert all(g.num_train == 40 for g in sp.gpr_err)


def test_refused_settings_and_refits(G):
    pb, Z = _e2e("ds2")
    dyn = _sparse_dynamics(G, pb, Z)
    with pytest.raises(ValueError, match="max_train"):
        dyn.max_train = 100
    with pytest.raises(ValueError, match="async_rebuild"):
        dyn.append_train_data(pb["X"][0, :2], pb["X"][0, 2:], pb["Y"][0], async_rebuild=True)
    mpc = G.RiskSensitiveMPC(-1.0, 5, 2, 1, pb["Q"], pb["R"])
    mpc.dynamics = dyn
    with pytest.raises(ValueError, match="max_train"):
        G.Simulator(mpc, None, max_train=50)
    cost = G.CostParams(-1.0, pb["Q"], pb["R"])
    p0 = dyn.pack()
    r0 = dyn.rollout(pb["x0"], pb["U"], cost)["cost"].cpu().numpy()
    # a hyper-parameter change and other inducing points refit from the kept data; the same M keeps the pack
    dyn.gpr_err[0].set_sigma_n(2e-2)
    r1 = dyn.rollout(pb["x0"], pb["U"], cost)["cost"].cpu().numpy()
    assert dyn.pack() is p0 and not np.array_equal(r0, r1)
    dyn.gpr_err[0].set_sigma_n(float(pb["sigma_n"][0]))
    np.testing.assert_allclose(dyn.rollout(pb["x0"], pb["U"], cost)["cost"].cpu().numpy(), r0, rtol=1e-12)
    Z2 = G.select_inducing(pb["X"], 32, pb["lambdas"][0])
    dyn.set_inducing(Z2)
    assert dyn.pack() is p0 and np.all(np.isfinite(dyn.rollout(pb["x0"], pb["U"], cost)["cost"].cpu().numpy()))
    dyn.set_inducing(Z2[:20])                                                # (another M within the padded size: resized in place)
    assert dyn.pack().N == 20 and np.all(np.isfinite(dyn.rollout(pb["x0"], pb["U"], cost)["cost"].cpu().numpy()))
    dyn.set_inducing(G.select_inducing(pb["X"], 70, pb["lambdas"][0]))       # beyond it: a new pack
    assert dyn.pack() is not p0 and dyn.pack().N == 70
    # without the data neither is possible
    nd = _sparse_dynamics(G, pb, Z, keep_data=False)
    nd.pack()
    with pytest.raises(RuntimeError, match="keep_data"):
        nd.set_inducing(Z2)
    nd.gpr_err[1].set_sigma_n(3e-2)
    with pytest.raises(RuntimeError, match="keep_data"):
        nd.pack()


def test_shared_hyperparameters_share_one_state_and_nominal_residuals(G):
    """GPs with bit-identical hyper-parameters share W, G, Binv, Q (their targets are columns of one r); with the identity nominal model the
    accumulators see the residuals: the result equals a fit without a model on targets Y - x."""
    pb, Z = _e2e("ds2")
    lam = pb["lambdas"][0]

    def make(nominal, Y):
        dyn = G.SparseDynamics(2, 1, Z, nominal_models=nominal)
        for g in dyn.gpr_err:
            g.set_lambdas(lam)
            g.set_sigma_n(1e-2)
        dyn.append_train_data(pb["X"][:, :2], pb["X"][:, 2:], Y)
        return dyn
    a = make(G.LinearNominalModel.identity(2, 1), pb["Y"])
    b = make(None, pb["Y"] - pb["X"][:, :2])
    assert len(a._groups) == 1 and a._groups[0][0] == [0, 1] and a.posterior()[1].dim() == 2
    np.testing.assert_allclose(a.posterior()[0].cpu().numpy(), b.posterior()[0].cpu().numpy(), rtol=0, atol=1e-9)
    assert a.pack().nominal is not None and b.pack().nominal is None
    cost = G.CostParams(-1.0, pb["Q"], pb["R"])
    ra, rb = a.rollout(pb["x0"], pb["U"], cost), b.rollout(pb["x0"], pb["U"], cost)
    assert np.all(np.isfinite(ra["cost"].cpu().numpy())) and not np.allclose(ra["means"].cpu().numpy(), rb["means"].cpu().numpy())


@pytest.mark.parametrize("solver", [None, "mppi", "lbfgs"])
def test_pendulum_closed_loop(G, solver):
    """30 steps with M = 32 and the identity nominal model: num_train grows, ONE pack handle, ONE capture of the callback graph."""
    from gaussian_process_mpc_amd._lib import lib
    rng = np.random.default_rng(3)
    plant = G.PendulumPlant(init_state=(0.3, 0.0))
    S = np.stack((rng.uniform(-1, 1, 40), rng.uniform(-2, 2, 40)), axis=1)
    A = rng.uniform(-2, 2, (40, 1))
    nxt = np.array([G.PendulumPlant(init_state=s).step(a)[0] for s, a in zip(S, A)])
    mpc = G.RiskSensitiveMPC(-1.0, 5, 2, 1, 0.5 * np.eye(2), 0.01 * np.eye(1), nominal_models=G.LinearNominalModel.identity(2, 1))
    for g in mpc.dynamics.gpr_err:
        g.set_lambdas(np.array([1.0, 4.0, 4.0]))
        g.set_sigma_n(np.array(1e-2))
    box = np.array([[-1.5, -3.0, -2.0], [1.5, 3.0, 2.0]])
    Z = G.select_inducing(rng.uniform(box[0], box[1], (400, 3)), 32, np.array([1.0, 4.0, 4.0]))
    dyn = mpc.use_inducing_points(Z)
    assert isinstance(dyn, G.SparseDynamics) and dyn is mpc.dynamics and dyn.nominal_models is not None
    dyn.append_train_data(S, A, nxt)
    mpc.set_lb([-2.0]); mpc.set_ub([2.0])
    mpc.solver = solver
    p0 = dyn.pack()
    h0 = p0.handle
    assert p0.N == 32 and p0.nominal is not None
    steps = 30
    hist = G.Simulator(mpc, plant, num_iters=steps, incremental=True).run()
    assert len(hist) == steps and all(np.isfinite(h[2]) for h in hist) and all(abs(h[1][0]) <= 2.0 + 1e-9 for h in hist)
    assert dyn.num_train == 40 + steps == dyn.gpr_err[0].num_train == dyn._groups[0][1].num_obs
    p1 = dyn.pack()
    assert p1 is p0 and p1.handle is h0 and p1.N == 32
    if solver is None:
        assert lib().gpmpc_pack_callback_captures(h0) == 1
    mpc.curr_state = torch.tensor(hist[-1][0], dtype=torch.float64, device=mpc.device)
    mpc._cache_key = None
    assert np.isfinite(mpc.objective(0.5 * np.ones(5)))
    assert dyn._groups[0][1].min_lambda > 0
