"""The sparse-GP window on the device against tests/sparse_window_reference.py: gpmpc_sparse_remove, gpmpc_sparse_replace,
SparseGPState.remove / replace / rebase and SparseDynamics(window=...).

Kernel level: the ladder of tests/sparse_reference.py, the float64 state rounded from the extended-precision fit (as the append test
builds it), row n / 2 removed and replaced, a padded ld_w in a NaN-filled buffer, alpha pre-filled with NaN, guarded workspaces.  Every
output is held under ``allowance4``: max(8 e64, 1e-13 max|ref|) with e64 the largest error of FOUR float64 evaluations in different
summation orders (a removal cancels; tests/test_host_sparse_window.py shows that one evaluation's error is no fair measure and that
unseen float64 evaluations stay inside this rule).  The bit-for-bit properties the header promises are asserted as such.

Chain: 300 replacements in ring order on a window of 48 rows against the extended-precision BATCH fit of the last 48, under
allowance4 of four float64 CHAINS (the drift of a chain is a property of the recursion in float64, not of the device: DESIGN.md
section 3h), with and without a rebase every 48.

End to end: SparseDynamics(window=48) at the project's end-to-end tolerances against the reference rollout on the batch fit of the
rows the window holds."""
import functools

import numpy as np
import pytest
import torch

import sparse_reference as R
import sparse_window_reference as WR
import test_gpu_sparse as T
from test_gpu_sparse import _L, _Workspace, _check, _dev, _lp, _nan, _padded, _same_bits, _sp, _vp

pytestmark = pytest.mark.gpu

E_ARG, E_WORKSPACE = -1, -4
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


def _call(name, pr, st, rows, ld_w=None, stats=(0.0, 7.0), nt=None, refuse_short=True):
    """One gpmpc_sparse_<name> call on device copies of the float64 state ``st``; rows: the host vectors x_old, y_old[, x_new, y_new].
    Returns the device tensors G, r, Binv, Q, alpha, stats."""
    M, D = pr["M"], pr["D"]
    nt = st["r"].shape[1] if nt is None else nt
    ld_w = ld_w or M + 5
    W, Z = _padded(pr["W"], ld_w), _dev(pr["Z"])
    out = {"G": _dev(st["G"]), "r": _dev(st["r"][:, :nt]), "Binv": _dev(st["Binv"]), "Q": _dev(st["Q"]), "alpha": _nan(M, nt),
           "stats": _dev(stats)}
    vecs = [_dev(np.asarray(a)[:nt] if i % 2 else a) for i, a in enumerate(rows)]
    nb = getattr(_L(), "gpmpc_sparse_%s_workspace_bytes" % name)(M, nt)
    ws = _Workspace(nb)
    fn = getattr(_L(), "gpmpc_sparse_" + name)
    args = (D, M, nt, *[_vp(v) for v in vecs], _vp(Z), _vp(W), ld_w, _lp(pr["lam"])[1], pr["sf"], pr["noise"],
            *[_vp(out[k]) for k in ("G", "r", "Binv", "Q", "alpha", "stats")], ws.ptr)
    if refuse_short:
        assert fn(*args, nb - 1, _sp()) == E_WORKSPACE
    _check(fn(*args, nb, _sp()), "gpmpc_sparse_" + name)
    ws.assert_guard_intact()
    return out


def _hold(name, got, ref, k, label):
    allow = WR.allowance4(ref["ld"][k], [f[k] for f in ref["f64"]])
    e = R.err(got, ref["ld"][k])
    print("  %-34s %-6s err %.2e allowance %.2e (%.3f)" % (label, k, e, allow, e / allow))
    assert _note(name, e / allow) <= 1, (label, k, e, allow)


# ------------------------------------------------------------------------------------------------------------------ kernel ladder
@pytest.mark.parametrize("M,n,D,nt", R.ladder())
def test_remove_replace_ladder(G, M, n, D, nt):
    (pr, st), j = WR.problem(M, n, D, nt), n // 2
    c = WR.case(M, n, D, nt, j)
    label = "M %3d n %3d D %d nt %d row %d" % (M, n, D, nt, j)
    rem = _call("remove", pr, st, (pr["X"][j], pr["Y"][j]), stats=(float(n), 7.0))
    for k in WR.OUTPUTS:
        _hold("remove", rem[k].cpu().numpy(), c["rem"], k, "remove  " + label)
    assert rem["stats"].tolist() == [float(n - 1), 7.0]                      # stats[1] is left alone: a lower bound from here on
    assert _same_bits(rem["G"], rem["G"].T) and _same_bits(rem["Binv"], rem["Binv"].T) and _same_bits(rem["Q"], rem["Q"].T)
    if n == 1:
        # the only row leaves: G -> 0, Q -> 0 and Binv -> I, each as far as the allowance above says.  For G that is plain: Lambda is a
        # cancelling difference with a float64 relative error of 1e-11 ... 3e-10, so v v^T / Lambda meets the stored G to
        # that, times its size (1e-9: three times the larger figure)
        assert float(rem["G"].abs().max()) <= 1e-9 * float(np.abs(st["G"]).max())
    rep = _call("replace", pr, st, (pr["X"][j], pr["Y"][j], pr["xnew"], pr["ynew"]), stats=(float(n), 7.0))
    for k in WR.OUTPUTS:
        _hold("replace", rep[k].cpu().numpy(), c["rep"], k, "replace " + label)
    lam_ref = {"ld": {"Lambda": np.array([c["rep"]["ld"]["Lambda"]])}, "f64": [{"Lambda": np.array([f["Lambda"]])} for f in c["rep"]["f64"]]}
    _hold("replace", rep["stats"][1:].cpu().numpy(), lam_ref, "Lambda", "replace " + label)   # (7.0 is above every Lambda here)
    assert rep["stats"][0].item() == float(n)
    assert _same_bits(rep["G"], rep["G"].T) and _same_bits(rep["Binv"], rep["Binv"].T) and _same_bits(rep["Q"], rep["Q"].T)


# ------------------------------------------------------------------------------------------------------------------ bit-for-bit properties
def _append_onto(pr, dev, ld_w):
    """gpmpc_sparse_append of (xnew, ynew) onto the device state ``dev`` (in place)."""
    M, D, nt = pr["M"], pr["D"], dev["r"].shape[1]
    W, Z, x, y = _padded(pr["W"], ld_w), _dev(pr["Z"]), _dev(pr["xnew"]), _dev(pr["ynew"][:nt])
    nb = _L().gpmpc_sparse_append_workspace_bytes(M, nt)
    ws = _Workspace(nb)
    _check(_L().gpmpc_sparse_append(D, M, nt, _vp(x), _vp(y), _vp(Z), _vp(W), ld_w, _lp(pr["lam"])[1], pr["sf"], pr["noise"],
                                    *[_vp(dev[k]) for k in ("G", "r", "Binv", "Q", "alpha", "stats")], ws.ptr, nb, _sp()), "gpmpc_sparse_append")
    ws.assert_guard_intact()
    return dev


@pytest.mark.parametrize("M,n,D", [(33, 200, 5), (130, 200, 2), (16, 65, 8)])
def test_remove_replace_bit_properties(G, M, n, D):
    (pr, st), j = WR.problem(M, n, D, 4), n // 2
    old, both = (pr["X"][j], pr["Y"][j]), (pr["X"][j], pr["Y"][j], pr["xnew"], pr["ynew"])
    keys = WR.OUTPUTS + ("stats",)
    for name, rows in (("remove", old), ("replace", both)):
        a = _call(name, pr, st, rows, stats=(float(n), 7.0))
        b = _call(name, pr, st, rows, stats=(float(n), 7.0))
        c = _call(name, pr, st, rows, ld_w=M + 11, stats=(float(n), 7.0))
        d = _call(name, pr, st, rows, ld_w=M, stats=(float(n), 7.0))
        for k in keys:
            assert _same_bits(a[k], b[k]) and _same_bits(a[k], c[k]) and _same_bits(a[k], d[k]), (name, k)   # identical calls; ld_w does not matter
        for k in ("G", "Binv", "Q"):
            assert _same_bits(a[k], a[k].T), (name, k)
        # column a of r (and of alpha) does not depend on the other targets
        one = _call(name, pr, st, rows, nt=1, stats=(float(n), 7.0))
        assert _same_bits(one["r"][:, 0], a["r"][:, 0]) and _same_bits(one["alpha"][:, 0], a["alpha"][:, 0]) and _same_bits(one["G"], a["G"]), name
        Y2, y2 = np.array(pr["Y"][j]), np.array(pr["ynew"])
        Y2[[0, 1, 3]] *= 1e3
        y2[[0, 1, 3]] -= 5.0
        other = _call(name, pr, st, (rows[0], Y2) + ((rows[2], y2) if len(rows) == 4 else ()), stats=(float(n), 7.0))
        assert _same_bits(other["r"][:, 2], a["r"][:, 2]) and not _same_bits(other["r"][:, 1], a["r"][:, 1]), name
    # G and r of a replace are those of remove followed by append, bit for bit; Binv, Q, alpha agree to rounding
    rep = _call("replace", pr, st, both, stats=(float(n), 7.0))
    two = _append_onto(pr, _call("remove", pr, st, old, stats=(float(n), 7.0)), M + 5)
    assert _same_bits(rep["G"], two["G"]) and _same_bits(rep["r"], two["r"])
    assert rep["stats"][0].item() == two["stats"][0].item() == float(n) and _same_bits(rep["stats"][1:], two["stats"][1:])
    for k in ("Binv", "Q", "alpha"):
        assert float((rep[k] - two[k]).abs().max()) <= 1e-9 * max(1.0, float(two[k].abs().max())), k
    # a minimum below the new Lambda stays; NaN is passed on
    assert _call("replace", pr, st, both, stats=(float(n), 1e-9))["stats"].tolist() == [float(n), 1e-9]
    assert np.isnan(_call("replace", pr, st, both, stats=(float(n), float("nan")))["stats"][1].item())


def test_refusals_with_device_buffers(G):
    M, n, D, nt = 16, 65, 8, 4
    pr, st = WR.problem(M, n, D, nt)
    dev = {k: _dev(st[k]) for k in ("G", "r", "Binv", "Q")}
    dev.update(alpha=_dev(np.ones((M, nt))), stats=_dev([float(n), 0.5]))
    before = {k: v.clone() for k, v in dev.items()}
    W, Z = _dev(pr["W"]), _dev(pr["Z"])
    x, y, xn, yn = _dev(pr["X"][3]), _dev(pr["Y"][3]), _dev(pr["xnew"]), _dev(pr["ynew"])
    for name, vecs in (("remove", (x, y)), ("replace", (x, y, xn, yn))):
        fn = getattr(_L(), "gpmpc_sparse_" + name)
        ws = _Workspace(getattr(_L(), "gpmpc_sparse_%s_workspace_bytes" % name)(M, nt))
        for kw in (dict(M=0), dict(M=8193), dict(D=9), dict(D=0), dict(nt=9), dict(nt=0), dict(ld_w=M - 1), dict(null=0), dict(null=len(vecs) - 1)):
            a = dict(D=D, M=M, nt=nt, ld_w=M, null=None)
            a.update(kw)
            v = [None if i == a["null"] else t for i, t in enumerate(vecs)]
            rc = fn(a["D"], a["M"], a["nt"], *[_vp(t) for t in v], _vp(Z), _vp(W), a["ld_w"], _lp(pr["lam"])[1], pr["sf"], pr["noise"],
                    *[_vp(dev[k]) for k in ("G", "r", "Binv", "Q", "alpha", "stats")], ws.ptr, ws.nbytes, _sp())
            assert rc == E_ARG and _L().gpmpc_last_error().decode().startswith("gpmpc_sparse_" + name), (name, kw)
        torch.cuda.synchronize()
        ws.assert_guard_intact()
        for k in dev:
            assert _same_bits(dev[k], before[k]), (name, k)                  # refused before any launch


# ------------------------------------------------------------------------------------------------------------------ chain of replacements
CHAIN = dict(M=33, window=48, steps=300, D=3, nt=2)


@functools.lru_cache(maxsize=None)
def _chain_problem(sigma_n):
    c = CHAIN
    return R.problem(4242, c["window"] + c["steps"], c["M"], c["D"], c["nt"], sigma_n=sigma_n)


@pytest.mark.parametrize("rebase_every", [0, 48], ids=["no_rebase", "rebase_48"])
@pytest.mark.parametrize("sigma_n", [1e-2, 0.1])
def test_chain_of_replacements(G, sigma_n, rebase_every):
    """48 rows fitted, 300 replacements in ring order (refresh_every = 64), against the extended-precision batch fit of the last 48 rows
    under allowance4 of the four float64 chains with the same counters; the W the state built is data for the reference."""
    pr, w = _chain_problem(sigma_n), CHAIN["window"]
    hyp = (pr["lam"], pr["sf"], pr["noise"])
    st = G.SparseGPState(pr["Z"], pr["lam"], pr["sf"], sigma_n)
    assert st.refresh_every == 64
    X, Y = _dev(pr["X"]), _dev(pr["Y"])
    st.fit(X[:w], Y[:w])
    tensors = {k: getattr(st, k).data_ptr() for k in WR.OUTPUTS}
    W = st.W.cpu().numpy()
    n, checked = pr["n"], 0
    for i in range(w, n):
        st.replace(X[i - w], Y[i - w], X[i], Y[i])
        if rebase_every and (i - w + 1) % rebase_every == 0:
            st.rebase(X[i - w + 1:i + 1], Y[i - w + 1:i + 1])
            if i - w + 1 in (rebase_every, (CHAIN["steps"] // rebase_every) * rebase_every):     # the first and the last rebase
                lo, hi = i - w + 1, i + 1
                fresh = G.SparseGPState(pr["Z"], pr["lam"], pr["sf"], sigma_n).fit(X[lo:hi], Y[lo:hi])
                ld = R.fit(pr["X"][lo:hi], pr["Y"][lo:hi], pr["Z"], *hyp, st.jitter, W=W)
                f64 = R.fit(pr["X"][lo:hi], pr["Y"][lo:hi], pr["Z"], *hyp, st.jitter, W=W, prec=np.float64)
                for k in WR.OUTPUTS:
                    assert _same_bits(getattr(st, k), getattr(fresh, k)), k                  # rebase == fit on the same rows, bit for bit
                    allow, e = R.allowance(ld[k], f64[k]), R.err(getattr(st, k).cpu().numpy(), ld[k])
                    print("  sigma_n %.0e right after the rebase at %3d, %-5s err %.2e allowance %.2e (%.3f)" % (sigma_n, lo, k, e, allow, e / allow))
                    assert _note("rebase_vs_batch", e / allow) <= 1, k
                assert st.num_obs == w
                checked += 1
    assert checked == (2 if rebase_every else 0)
    assert st.num_obs == w and all(getattr(st, k).data_ptr() == p for k, p in tensors.items())          # in place throughout
    assert _same_bits(st.G, st.G.T) and _same_bits(st.Binv, st.Binv.T) and _same_bits(st.Q, st.Q.T)
    ld = R.fit(pr["X"][n - w:], pr["Y"][n - w:], pr["Z"], *hyp, st.jitter, W=W)
    chains = [WR.chain(pr["X"], pr["Y"], pr["Z"], W, *hyp, w, prec=np.float64, order=o, refresh_every=64, rebase_every=rebase_every)
              for o in WR.ORDERS]
    for k in WR.OUTPUTS:
        allow, e = WR.allowance4(ld[k], [c[k] for c in chains]), R.err(getattr(st, k).cpu().numpy(), ld[k])
        e64 = [R.err(c[k], ld[k]) for c in chains]
        print("  sigma_n %.0e rebase_every %2d: 300 replacements against the batch fit, %-5s err %.2e (float64 chains %.2e ... %.2e) "
              "allowance %.2e (%.3f)" % (sigma_n, rebase_every, k, e, min(e64), max(e64), allow, e / allow))
        assert _note("chain_rebase" if rebase_every else "chain", e / allow) <= 1, k


# ------------------------------------------------------------------------------------------------------------------ SparseDynamics(window=...)
WINDOW = 48


def _hypers(dyn, pb, shared=False, sigma_n=None):
    for a, g in enumerate(dyn.gpr_err):
        g.set_lambdas(pb["lambdas"][0 if shared else a])
        g.set_sigma_n(float(pb["sigma_n"][0 if shared else a]) if sigma_n is None else sigma_n)
        g.set_sigma_f(1.0)


def _feed(dyn, pb, lo, hi, single):
    ds = pb["ds"]
    if not single:
        dyn.append_train_data(pb["X"][lo:hi, :ds], pb["X"][lo:hi, ds:], pb["Y"][lo:hi])
        return
    for i in range(lo, hi):
        dyn.append_train_data(pb["X"][i, :ds], pb["X"][i, ds:], pb["Y"][i])


def _ring_rows(dyn):
    X, Y = dyn._rows()
    return X.cpu().numpy(), Y.cpu().numpy()


def test_window_dynamics_end_to_end(G):
    """A window of 48 filled in bulk, then 150 single observations: num_train stays 48, the pack handle and the ONE captured callback
    graph are those built first, and the rollout is the reference rollout on the batch fit of the last 48 rows (two hyper-parameter
    groups: the GPs' length-scales differ)."""
    from gaussian_process_mpc_amd._lib import lib
    pb, Z = T._e2e("ds2")
    dyn = G.SparseDynamics(pb["ds"], pb["da"], Z, window=WINDOW)
    assert dyn.window == WINDOW and dyn.window_slot == 0 and dyn.rebase_every == WINDOW and dyn.max_train is None
    _hypers(dyn, pb)
    _feed(dyn, pb, 0, 20, single=False)
    _feed(dyn, pb, 20, WINDOW, single=True)                                  # below the window: behaviour as without one
    assert dyn.num_train == WINDOW and dyn.window_slot == 0 and len(dyn._groups) == 2
    mpc = G.RiskSensitiveMPC(-1.0, pb["H"], pb["ds"], pb["da"], pb["Q"], pb["R"])
    mpc.dynamics = dyn
    mpc.curr_state = torch.tensor(pb["x0"][0], dtype=torch.float64, device=mpc.device)
    p0 = dyn.pack()
    h0 = p0.handle
    assert np.isfinite(mpc.objective(pb["U"][0].reshape(-1)))
    assert lib().gpmpc_pack_callback_captures(h0) == 1
    xbuf = dyn._Xbuf.data_ptr()
    for lo in range(WINDOW, WINDOW + 150, 50):
        _feed(dyn, pb, lo, lo + 50, single=True)
        mpc._cache_key = None
        assert np.isfinite(mpc.objective(pb["U"][0].reshape(-1)))
    last = WINDOW + 150
    assert dyn.num_train == WINDOW == dyn.gpr_err[0].num_train and dyn.window_slot == 150 % WINDOW and dyn._Xbuf.shape[0] == WINDOW
    assert all(st.num_obs == WINDOW for _, st in dyn._groups) and dyn._Xbuf.data_ptr() == xbuf
    assert dyn.pack() is p0 and dyn.pack().handle is h0 and lib().gpmpc_pack_callback_captures(h0) == 1
    Xr, Yr = _ring_rows(dyn)
    assert np.array_equal(Xr, pb["X"][last - WINDOW:last]) and np.array_equal(Yr, pb["Y"][last - WINDOW:last])
    pe = dict(T._effective(pb, dyn), X=pb["X"][last - WINDOW:last], Y=pb["Y"][last - WINDOW:last])
    alpha, Q = R.fit_bundle(pe, Z)
    cost = G.CostParams(-1.0, pb["Q"], pb["R"])
    r = dyn.rollout(pb["x0"], pb["U"], cost, want_grad=True)
    torch.cuda.synchronize()
    for b in range(pb["B"]):
        ref = R.rollout(Z, alpha, Q, pe["lambdas"], pe["sigma_f"], pb["H"], pb["x0"][b], pb["U"][b], pb["Q"], pb["R"], -1.0)
        T._assert_e2e({k: v[b].cpu().numpy() for k, v in r.items()}, ref, ("means", "vars", "cost", "grad"), "window 48 after 150, traj %d" % b)
    # a bulk load into the full window keeps the newest 48 rows, oldest first, and refits
    _feed(dyn, pb, last, last + 30, single=False)
    Xr, Yr = _ring_rows(dyn)
    assert dyn.num_train == WINDOW and dyn.window_slot == 0 and np.array_equal(Xr, pb["X"][last + 30 - WINDOW:last + 30])
    assert np.array_equal(Yr, pb["Y"][last + 30 - WINDOW:last + 30]) and dyn.pack() is p0
    fresh = G.SparseDynamics(pb["ds"], pb["da"], Z)
    _hypers(fresh, pb)
    _feed(fresh, pb, last + 30 - WINDOW, last + 30, single=False)
    c_win, c_fresh = (d.rollout(pb["x0"], pb["U"], cost)["cost"].cpu().numpy() for d in (dyn, fresh))
    np.testing.assert_allclose(c_win, c_fresh, rtol=1e-12)                   # (the same rows through the same fit)
    # a hyper-parameter change refits from the ring (here after the ring has wrapped again)
    _feed(dyn, pb, last + 30, last + 37, single=True)
    assert dyn.window_slot == 7
    dyn.gpr_err[0].set_sigma_n(2e-2)
    fresh = G.SparseDynamics(pb["ds"], pb["da"], Z)
    _hypers(fresh, pb)
    fresh.gpr_err[0].set_sigma_n(2e-2)
    _feed(fresh, pb, last + 37 - WINDOW, last + 37, single=False)
    c_win, c_fresh = (d.rollout(pb["x0"], pb["U"], cost)["cost"].cpu().numpy() for d in (dyn, fresh))
    np.testing.assert_allclose(c_win, c_fresh, rtol=1e-12)
    assert dyn.pack() is p0 and dyn.num_train == WINDOW
    # a first bulk load larger than the window
    big = G.SparseDynamics(pb["ds"], pb["da"], Z, window=WINDOW)
    _hypers(big, pb)
    _feed(big, pb, 0, 100, single=False)
    assert big.num_train == WINDOW and big.window_slot == 0 and np.array_equal(_ring_rows(big)[0], pb["X"][100 - WINDOW:100])


def test_window_dynamics_identity_nominal_one_group(G):
    """The identity nominal model and ONE hyper-parameter group (both GPs share r's columns): the replacement sees the residual of the
    old row as of the new one.  Against dynamics without a window, bulk-fitted on the rows the window holds, at the end-to-end figures."""
    pb, Z = T._e2e("ds2")
    nominal = G.LinearNominalModel.identity(2, 1)
    dyn = G.SparseDynamics(2, 1, Z, nominal_models=nominal, window=WINDOW)
    _hypers(dyn, pb, shared=True, sigma_n=1e-2)
    _feed(dyn, pb, 0, WINDOW, single=False)
    p0 = dyn.pack()
    _feed(dyn, pb, WINDOW, WINDOW + 150, single=True)
    last = WINDOW + 150
    assert len(dyn._groups) == 1 and dyn.num_train == WINDOW and dyn.pack() is p0 and p0.nominal is not None
    fresh = G.SparseDynamics(2, 1, Z, nominal_models=nominal)
    _hypers(fresh, pb, shared=True, sigma_n=1e-2)
    _feed(fresh, pb, last - WINDOW, last, single=False)
    cost = G.CostParams(-1.0, pb["Q"], pb["R"])
    rw, rf = dyn.rollout(pb["x0"], pb["U"], cost, want_grad=True), fresh.rollout(pb["x0"], pb["U"], cost, want_grad=True)
    for b in range(pb["B"]):
        T._assert_e2e({k: v[b].cpu().numpy() for k, v in rw.items()}, {k: v[b].cpu().numpy() for k, v in rf.items()},
                      ("means", "vars", "cost", "grad"), "window 48, identity nominal, traj %d" % b)
    # ... and the accumulators saw residuals: without the model on targets Y - x the posterior is the same
    plain = G.SparseDynamics(2, 1, Z)
    _hypers(plain, pb, shared=True, sigma_n=1e-2)
    plain.append_train_data(pb["X"][last - WINDOW:last, :2], pb["X"][last - WINDOW:last, 2:], pb["Y"][last - WINDOW:last] - pb["X"][last - WINDOW:last, :2])
    np.testing.assert_allclose(plain.posterior()[0].cpu().numpy(), fresh.posterior()[0].cpu().numpy(), rtol=0, atol=1e-9)


def test_window_refusals(G):
    pb, Z = T._e2e("ds2")
    with pytest.raises(ValueError, match="keep_data"):
        G.SparseDynamics(2, 1, Z, window=WINDOW, keep_data=False)
    with pytest.raises(ValueError, match="window"):
        G.SparseDynamics(2, 1, Z, window=0)
    dyn = G.SparseDynamics(2, 1, Z, window=WINDOW)
    with pytest.raises(ValueError, match="max_train"):
        dyn.max_train = 100
    mpc = G.RiskSensitiveMPC(-1.0, 5, 2, 1, pb["Q"], pb["R"])
    assert mpc.use_inducing_points(Z, window=WINDOW).window == WINDOW and mpc.use_inducing_points(Z).window is None
    mpc.use_inducing_points(Z, window=WINDOW)
    with pytest.raises(ValueError, match="max_train"):
        G.Simulator(mpc, None, max_train=50)
    st = G.SparseGPState(Z, pb["lambdas"][0], 1.0, 1e-2)
    for call in (lambda: st.remove(pb["X"][0], pb["Y"][0, :1]), lambda: st.rebase(pb["X"][:4], pb["Y"][:4, :1]),
                 lambda: st.replace(pb["X"][0], pb["Y"][0, :1], pb["X"][1], pb["Y"][1, :1])):
        with pytest.raises(RuntimeError, match="no data"):
            call()
    st.fit(pb["X"][:10], pb["Y"][:10, :1])
    with pytest.raises(ValueError, match="remove takes"):
        st.remove(pb["X"][0, :2], pb["Y"][0, :1])
    st.remove(pb["X"][3], pb["Y"][3, :1])
    assert st.num_obs == 9


def test_pendulum_closed_loop_with_a_window(G):
    """25 steps with M = 32, the identity nominal model and a window of 40 that is full from the start: every step replaces, num_train
    stays 40, ONE pack handle, ONE capture of the callback graph."""
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
    dyn = mpc.use_inducing_points(Z, window=40)
    assert dyn.window == 40 and dyn is mpc.dynamics
    dyn.append_train_data(S, A, nxt)
    mpc.set_lb([-2.0]); mpc.set_ub([2.0])
    p0 = dyn.pack()
    h0 = p0.handle
    steps = 25
    hist = G.Simulator(mpc, plant, num_iters=steps, incremental=True).run()
    assert len(hist) == steps and all(np.isfinite(h[2]) for h in hist) and all(abs(h[1][0]) <= 2.0 + 1e-9 for h in hist)
    assert dyn.num_train == 40 == dyn.gpr_err[0].num_train == dyn._groups[0][1].num_obs and dyn.window_slot == steps % 40
    assert dyn.pack() is p0 and dyn.pack().handle is h0 and p0.N == 32 and lib().gpmpc_pack_callback_captures(h0) == 1
    assert np.all(np.isfinite(dyn.posterior()[0].cpu().numpy()))
