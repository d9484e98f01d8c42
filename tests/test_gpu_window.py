"""GPU tests of the fixed-size training window: removal and replacement of ONE training point in O(N^2) (C ABI gpmpc_kinv_remove,
gpmpc_gp_replace), GaussianProcessRegression.remove_train_data / replace_train_data, Dynamics.max_train and the windowed closed
loop.  The reference has no such update; like the Schur append it is pinned to the reference through what ``build_Ky_inv_mat`` gives
on the same rows (the golden fixtures), and the tolerances are those of the named tests of the append in tests/test_gpu_api.py."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    return g


def _g6_gp(G, z, X, y):
    gp = G.GaussianProcessRegression(3)
    gp.set_lambdas(z["lam"]); gp.set_sigma_f(1.4); gp.set_sigma_n(0.2)      # hypers of test_incremental_append_matches_rebuild
    gp.append_train_data(X, y)
    return gp


def _against_g6_fixture(gp, z):
    assert gp.num_train == 64 and gp.Ky_inv.shape == (64, 64) and gp.X_train.shape == (64, 3) and gp.y_train.shape == (64, 1)
    np.testing.assert_allclose(gp.Ky.cpu().numpy(), z["Ky"], rtol=1e-12, atol=1e-14)
    scale = np.abs(z["Ky_inv"]).max()
    err = np.abs(gp.Ky_inv.cpu().numpy() - z["Ky_inv"]).max() / scale
    f, _ = gp.predict_latent_vars(z["Xp"])
    print("  Ky_inv against the fixture: %.3e of its largest element; mean rel. err %.3e" % (err, np.abs(f / z["f"] - 1).max()))
    assert err <= 1e-9
    np.testing.assert_allclose(f, z["f"], rtol=1e-8)
    return scale


@pytest.mark.parametrize("pos", [0, 30, 64])
def test_remove_matches_the_reference_fixture(G, golden, pos):
    """The 64 fixture rows with one extra row at `pos`; removing it in O(N^2) gives the matrices the reference built on the 64."""
    z = golden("g6_gp.npz")
    rng = np.random.default_rng(21)
    X, y = z["X"][:64], z["y"][:64].reshape(-1)
    extra_x, extra_y = rng.uniform(X.min(axis=0), X.max(axis=0)), float(rng.uniform(y.min(), y.max()))
    X65, y65 = np.insert(X, pos, extra_x, axis=0), np.insert(y, pos, extra_y)
    inc = _g6_gp(G, z, X65, y65)
    held = inc.Ky_inv
    held_copy = held.clone()
    inc.remove_train_data(pos, incremental=True)
    assert inc._appends_since_rebuild == 1                                   # the O(N^2) path, not a rebuild
    assert torch.equal(held, held_copy)                                      # nothing is modified under a holder
    np.testing.assert_array_equal(inc.X_train.cpu().numpy(), X)
    np.testing.assert_array_equal(inc.y_train.cpu().numpy().reshape(-1), y)
    _against_g6_fixture(inc, z)
    np.testing.assert_allclose(inc.Kf.cpu().numpy(), z["Kf"], rtol=1e-12, atol=1e-14)
    # incremental=False: the reference's own update on the remaining rows
    full = _g6_gp(G, z, X65, y65)
    full.remove_train_data(pos)
    fresh = _g6_gp(G, z, X, y)
    for name in ("X_train", "y_train", "Kf", "Ky", "Ky_inv"):
        assert torch.equal(getattr(full, name), getattr(fresh, name)), name
    assert full._appends_since_rebuild == 0
    with pytest.raises(IndexError):
        full.remove_train_data(64)


def test_replace_chain_matches_the_reference_fixture(G, golden):
    """Slots 0..13 start with other points and are overwritten, one by one, by the fixture's rows."""
    z = golden("g6_gp.npz")
    rng = np.random.default_rng(22)
    X, y = z["X"][:64], z["y"][:64].reshape(-1)
    X0, y0 = X.copy(), y.copy()
    X0[:14] = rng.uniform(X.min(axis=0), X.max(axis=0), (14, 3))
    y0[:14] = rng.uniform(y.min(), y.max(), 14)
    inc, full = _g6_gp(G, z, X0, y0), _g6_gp(G, z, X0, y0)
    for p in range(14):
        inc.replace_train_data(p, X[p], float(y[p]), incremental=True)
        full.replace_train_data(p, X[p], float(y[p]))
    assert inc._appends_since_rebuild == 14 and full._appends_since_rebuild == 0
    np.testing.assert_array_equal(inc.X_train.cpu().numpy(), X)
    np.testing.assert_array_equal(inc.y_train.cpu().numpy().reshape(-1), y)
    scale = _against_g6_fixture(inc, z)
    np.testing.assert_allclose(inc.Kf.cpu().numpy(), z["Kf"], rtol=1e-12, atol=1e-14)
    err = np.abs(inc.Ky_inv.cpu().numpy() - full.Ky_inv.cpu().numpy()).max() / scale
    print("  replace chain against the same chain of rebuilds: %.3e" % err)
    assert err <= 1e-10
    fresh = _g6_gp(G, z, X, y)
    assert torch.equal(full.Ky, fresh.Ky) and torch.equal(full.Ky_inv, fresh.Ky_inv)


def test_gp_replace_abi_padded_buffers_against_remove_then_append(G):
    """gpmpc_gp_replace called directly, inputs and outputs in buffers of (different) padded leading dimensions, against the
    composition gpmpc_kinv_remove -> gpmpc_kinv_append -> last row / column moved to `slot`, to 1e-12 of the largest element.
    The two forms round differently by about cond(Ky) * eps; the problem is that of test_gp_append_into_padded_buffers... with the
    noise of the g6 fixture (sigma_n = 0.2), where cond(Ky) <= n sigma_f^2 / sigma_n^2 = 2.7e3, i.e. 3e-13."""
    from gaussian_process_mpc_amd._lib import lib, ptr, stream_ptr, host_doubles, check
    dev = G.require_gpu()
    rng = np.random.default_rng(5)
    n, D, ld_i, cap = 75, 3, 96, 128
    X = torch.tensor(rng.uniform(-2, 2, (n + 1, D)), device=dev)
    lam, sf, noise = np.array([0.7, 1.3, 2.0]), 1.2, 0.2 ** 2
    _, lp = host_doubles(lam)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def kern(A, B):
        return sf ** 2 * torch.exp(-0.5 * ((A[:, None, :] - B[None, :, :]) ** 2 / torch.tensor(lam, device=dev)).sum(-1))

    eye = torch.eye(n, dtype=torch.float64, device=dev)
    Kf_old = kern(X[:n], X[:n])
    src = [torch.full((ld_i, ld_i), float("nan"), dtype=torch.float64, device=dev) for _ in range(3)]
    src[0][:n, :n], src[1][:n, :n], src[2][:n, :n] = Kf_old, Kf_old + noise * eye, torch.linalg.inv(Kf_old + noise * eye)
    src_copy = [t.clone() for t in src]
    X_old, xn = X[:n].contiguous(), X[n:n + 1].contiguous()
    nb = lib().gpmpc_gp_replace_workspace_bytes(n, D)
    ws = torch.empty(int(nb), dtype=torch.uint8, device=dev)
    for slot in (0, 20, n - 1):
        outs = []
        for rep in range(2):
            out = [torch.full((cap, cap), float("nan"), dtype=torch.float64, device=dev) for _ in range(3)]
            check(lib().gpmpc_gp_replace(n, D, slot, ptr(X_old), ptr(xn), lp, sf, noise, vp(src[0]), vp(src[1]), ld_i, vp(src[2]), ld_i,
                                         vp(out[0]), vp(out[1]), vp(out[2]), cap, vp(ws), ws.numel(), stream_ptr()), "gpmpc_gp_replace")
            outs.append(out)
        torch.cuda.synchronize()
        out = outs[0]
        for a, b in zip(outs[0], outs[1]):                               # fixed summation order: two calls, the same bits
            assert torch.equal(a[:n, :n], b[:n, :n])
        for a, b in zip(src, src_copy):                                  # inputs untouched (NaN padding included)
            assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))
        for t in out:                                                    # nothing beyond the n x n block is written
            assert torch.isnan(t[n:, :]).all() and torch.isnan(t[:, n:]).all() and not torch.isnan(t[:n, :n]).any()
        X_new = X_old.clone()
        X_new[slot] = xn[0]
        Kf_new = kern(X_new, X_new)
        np.testing.assert_allclose(out[0][:n, :n].cpu().numpy(), Kf_new.cpu().numpy(), rtol=1e-14, atol=1e-15)
        np.testing.assert_allclose(out[1][:n, :n].cpu().numpy(), (Kf_new + noise * eye).cpu().numpy(), rtol=1e-14, atol=1e-15)
        # the composition: remove `slot` (compacted), append the new point (last), move it to `slot`
        keep = [i for i in range(n) if i != slot]
        A = torch.full((n - 1, n - 1), float("nan"), dtype=torch.float64, device=dev)
        check(lib().gpmpc_kinv_remove(n, vp(src[2]), ld_i, slot, ptr(A), n - 1, stream_ptr()), "gpmpc_kinv_remove")
        k = out[0][slot, :n][keep].contiguous()                          # K_f(X without slot, x_new), held to torch above
        M = torch.empty((n, n), dtype=torch.float64, device=dev)
        nb2 = lib().gpmpc_kinv_append_workspace_bytes(n - 1)
        ws2 = torch.empty(int(nb2), dtype=torch.uint8, device=dev)
        check(lib().gpmpc_kinv_append(n - 1, ptr(A), ptr(k), sf ** 2 + noise, ptr(M), vp(ws2), ws2.numel(), stream_ptr()), "gpmpc_kinv_append")
        torch.cuda.synchronize()
        perm = torch.tensor(keep + [slot], device=dev)                   # position in M -> slot order
        R = torch.empty_like(M)
        R[perm[:, None], perm[None, :]] = M
        fresh = torch.linalg.inv(Kf_new + noise * eye)
        scale = float(fresh.abs().max())
        e_comp = float((out[2][:n, :n] - R).abs().max()) / scale
        e_fresh = float((out[2][:n, :n] - fresh).abs().max()) / scale
        print("  slot %2d: against remove + append %.3e, against a fresh inverse %.3e" % (slot, e_comp, e_fresh))
        assert e_comp <= 1e-12
        assert e_fresh <= 1e-9                                           # tolerance of the append's ABI test
    # the removal alone: the inverse of Ky without that row / column
    keep = [i for i in range(n) if i != 20]
    A = torch.empty((n - 1, n - 1), dtype=torch.float64, device=dev)
    check(lib().gpmpc_kinv_remove(n, vp(src[2]), ld_i, 20, ptr(A), n - 1, stream_ptr()), "gpmpc_kinv_remove")
    ref = torch.linalg.inv(src[1][:n, :n][keep][:, keep])
    assert float((A - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    # argument checks on real buffers: aliasing, leading dimension, slot
    call = lambda slot, o0, ldo: lib().gpmpc_gp_replace(n, D, slot, ptr(X_old), ptr(xn), lp, sf, noise, vp(src[0]), vp(src[1]), ld_i, vp(src[2]),  # noqa: E731
                                                       ld_i, vp(o0), vp(out[1]), vp(out[2]), ldo, vp(ws), ws.numel(), stream_ptr())
    assert call(0, src[0], cap) == -1 and call(0, out[0], n - 1) == -1 and call(n, out[0], cap) == -1


def _drift_stream(seed=11, D=3, n0=120, extra=380):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (n0 + extra, D))
    return X, np.sin(X).sum(axis=1), n0, extra


def _drift_gp(G, X, y):
    g = G.GaussianProcessRegression(X.shape[1])
    g.set_lambdas(np.array([1.5, 2.0, 1.0])); g.set_sigma_n(1e-2); g.set_sigma_f(1.2)   # regime of test_side_stream_rebuild_catches_up_and_swaps
    if len(X):
        g.append_train_data(X, y)
    return g


def test_replace_drift_is_bounded_by_the_periodic_rebuild(G):
    """380 first-in first-out replacements in a window of 120, default `rebuild_every`."""
    X, y, n0, extra = _drift_stream()
    inc = _drift_gp(G, X[:n0], y[:n0])
    Xw, yw = X[:n0].copy(), y[:n0].copy()
    rebuilds, worst = 0, 0.0
    for k in range(extra):
        slot = k % n0
        before = inc._appends_since_rebuild
        inc.replace_train_data(slot, X[n0 + k], float(y[n0 + k]), incremental=True)
        Xw[slot], yw[slot] = X[n0 + k], y[n0 + k]
        rebuilt = inc._appends_since_rebuild == 0
        assert rebuilt == (before >= inc.rebuild_every)
        rebuilds += int(rebuilt)
        if rebuilt or (k + 1) % 16 == 0 or k == extra - 1:
            ref = _drift_gp(G, Xw, yw)                                       # from scratch, on the window's rows in slot order
            assert inc.num_train == n0 and torch.equal(inc.X_train, ref.X_train) and torch.equal(inc.y_train, ref.y_train)
            if rebuilt:
                assert torch.equal(inc.Kf, ref.Kf) and torch.equal(inc.Ky, ref.Ky) and torch.equal(inc.Ky_inv, ref.Ky_inv)
            np.testing.assert_allclose(inc.Ky.cpu().numpy(), ref.Ky.cpu().numpy(), rtol=1e-13, atol=1e-15)
            np.testing.assert_allclose(inc.Kf.cpu().numpy(), ref.Kf.cpu().numpy(), rtol=1e-13, atol=1e-15)
            scale = float(ref.Ky_inv.abs().max())
            err = float((inc.Ky_inv - ref.Ky_inv).abs().max()) / scale
            worst = max(worst, err)
            assert err <= 5e-7, (k, err)
    print("  worst drift against a from-scratch inverse: %.3e of its largest element, %d rebuilds" % (worst, rebuilds))
    assert rebuilds == extra // (inc.rebuild_every + 1)


def test_replace_with_newton_refresh_never_rebuilds(G):
    """The same stream with refresh = "newton", rebuild_every = 16: a polish every 16 replacements, never a rebuild on a step."""
    X, y, n0, extra = _drift_stream()
    inc = _drift_gp(G, X[:n0], y[:n0])
    inc.rebuild_every, inc.refresh = 16, "newton"
    Xw = X[:n0].copy()
    refreshed, worst = 0, 0.0
    for k in range(extra):
        slot = k % n0
        v = inc.version
        inc.replace_train_data(slot, X[n0 + k], float(y[n0 + k]), incremental=True)
        Xw[slot] = X[n0 + k]
        if inc._appends_since_rebuild == 0:
            refreshed += 1
            assert inc.version == v + 2 and 1 <= inc.newton_steps_last <= 6       # replace + polish, not a rebuild
            fresh = torch.linalg.inv(inc.Ky)
            err = float((inc.Ky_inv - fresh).abs().max()) / float(fresh.abs().max())
            worst = max(worst, err)
            assert err <= 1e-7, (k, err)
        else:
            assert inc.version == v + 1
    print("  worst error right after a polish: %.3e of the largest element" % worst)
    assert refreshed == extra // 16
    ref = _drift_gp(G, Xw, np.zeros(n0))
    np.testing.assert_allclose(inc.Ky.cpu().numpy(), ref.Ky.cpu().numpy(), rtol=1e-13, atol=1e-15)


def test_window_holders_and_sharers(G):
    """Two GPs with identical hyper-parameters behind a Dynamics with a window: one set of matrices after windowed steps, nothing is
    modified under a holder during the step that follows, async_rebuild is refused."""
    rng = np.random.default_rng(5)
    dyn = G.Dynamics(2, 1)
    for gp in dyn.gpr_err:
        gp.set_lambdas(np.array([1.0, 2.0, 3.0])); gp.set_sigma_n(np.array(1e-2))
    S, A = rng.uniform(-1, 1, (30, 2)), rng.uniform(-1, 1, (30, 1))
    dyn.max_train = 30
    dyn.append_train_data(S, A, S + 0.1 * np.tanh(S))
    assert dyn.window_slot == 0
    lead, foll = dyn.gpr_err
    names = ("X_train", "y_train", "Kf", "Ky", "Ky_inv")
    for step in range(5):
        held = [(g, k, getattr(g, k), getattr(g, k).clone()) for g in dyn.gpr_err for k in names]
        s, a = rng.uniform(-1, 1, 2), rng.uniform(-1, 1, 1)
        dyn.append_train_data(s, a, s + 0.1 * np.tanh(s), incremental=True)
        assert dyn.window_slot == step + 1 and lead.num_train == foll.num_train == 30
        assert lead._appends_since_rebuild == foll._appends_since_rebuild == step + 1
        for k in ("X_train", "Kf", "Ky", "Ky_inv"):
            assert getattr(foll, k) is getattr(lead, k), k                   # shared
        assert foll.Ky_inv.untyped_storage().data_ptr() == lead.Ky_inv.untyped_storage().data_ptr()
        for g, k, t, c in held:
            assert getattr(g, k) is not t, k                                 # a new tensor ...
            assert torch.equal(t, c), k                                      # ... and the one held before the step kept its values
        np.testing.assert_array_equal(lead.X_train[step].cpu().numpy(), np.concatenate((s, a)))
        np.testing.assert_array_equal(np.array([g.y_train[step, 0].item() for g in dyn.gpr_err]), s + 0.1 * np.tanh(s))
    ref = G.GaussianProcessRegression(3)
    ref.set_lambdas(np.array([1.0, 2.0, 3.0])); ref.set_sigma_n(np.array(1e-2))
    ref.append_train_data(lead.X_train.cpu().numpy(), lead.y_train.cpu().numpy().reshape(-1))
    scale = float(ref.Ky_inv.abs().max())
    assert float((foll.Ky_inv - ref.Ky_inv).abs().max()) <= 5e-7 * scale
    # async_rebuild with a window: refused, and nothing was changed by the refused call
    X_before = lead.X_train
    s, a = rng.uniform(-1, 1, 2), rng.uniform(-1, 1, 1)
    with pytest.raises(ValueError):
        dyn.append_train_data(s, a, s, incremental=True, async_rebuild=True)
    assert lead.X_train is X_before and dyn.window_slot == 5 and not lead.async_rebuild
    lead.async_rebuild = True                                            # the same on a single GP
    with pytest.raises(ValueError):
        lead.replace_train_data(0, np.zeros(3), 0.0, incremental=True)
    with pytest.raises(ValueError):
        lead.remove_train_data(0, incremental=True)
    assert lead.X_train is X_before and lead.num_train == 30
    with pytest.raises(ValueError):
        G.Simulator(None, None, incremental=True, async_rebuild=True, max_train=30)


def _mpc_g3(G, z):
    N, ds, da, H = (int(v) for v in z["dims"])
    mpc = G.RiskSensitiveMPC(-1.0, H, ds, da, z["Q"], z["R"], z["R_delta"] if "R_delta" in z else None)
    _set_g3_hypers(mpc.dynamics, z)
    mpc.dynamics.append_train_data(z["X"][:, :ds], z["X"][:, ds:], z["Y"])
    for name, setter in (("x_ref", mpc.set_xref), ("u_ref", mpc.set_uref)):
        if name in z:
            setter(z[name])
    if "last_traj" in z:
        mpc.last_traj = z["last_traj"].copy()
    return mpc


def _set_g3_hypers(dyn, z):
    for a, g in enumerate(dyn.gpr_err):
        g.set_lambdas(z["lambdas"][a]); g.set_sigma_n(float(z["sigma_n"][a])); g.set_sigma_f(1.0)


def test_window_through_dynamics_and_the_solver_callbacks(G, golden):
    """g3 (N = 100, padded 128) with max_train = 100: 30 windowed steps keep the SAME pack object and the captured callback graph; the
    values are those of a from-scratch build on the window's rows in slot order."""
    from gaussian_process_mpc_amd._lib import lib
    from oracle import gpmpc_oracle as O
    z = golden("g3_rollout_c1.npz")
    N, ds, da, H = (int(v) for v in z["dims"])
    assert N == 100
    mpc, twin = _mpc_g3(G, z), _mpc_g3(G, z)
    dyn, tdyn = mpc.dynamics, twin.dynamics
    dyn.max_train = tdyn.max_train = 100
    for g in dyn.gpr_err:
        g.rebuild_every = 8
    mpc.curr_state = torch.tensor(z["x0"][0]).to(mpc.device)
    x = z["U"][0].reshape(-1).copy()
    p0 = dyn.pack()
    c_prev = mpc.objective(x)
    Xw, Yw = z["X"].copy(), z["Y"].copy()
    rng = np.random.default_rng(3)
    rebuilds, captures_after_first = 0, None
    worst_m, worst_v = 0.0, 0.0
    for k in range(30):
        s, a = rng.uniform(-1, 1, ds), rng.uniform(-1, 1, da)
        nxt = s + 0.1 * np.tanh(s) + 0.1 * a.sum()
        slot = dyn.window_slot
        assert slot == k % 100
        before = dyn.gpr_err[0]._appends_since_rebuild
        dyn.append_train_data(s, a, nxt, incremental=True)
        tdyn.append_train_data(s, a, nxt, incremental=False)
        Xw[slot], Yw[slot] = np.concatenate((s, a)), nxt
        assert all(g.num_train == 100 for g in dyn.gpr_err) and dyn.window_slot == (slot + 1) % 100
        assert dyn.pack() is p0 and p0.N == 100
        np.testing.assert_array_equal(dyn.gpr_err[0].X_train[slot].cpu().numpy(), Xw[slot])
        c = mpc.objective(x)
        assert c != c_prev                                               # same pack object, new contents: not served from the cache
        c_prev = c
        if k == 0:
            captures_after_first = lib().gpmpc_pack_callback_captures(p0.handle)
            assert captures_after_first >= 1                             # the callbacks above ran as the captured graph
        # from scratch, on the window's rows in slot order (through the same bulk path, so the same batched factorisation)
        scratch = G.Dynamics(ds, da)
        _set_g3_hypers(scratch, z)
        scratch.append_train_data(Xw[:, :ds], Xw[:, ds:], Yw)
        for g, t, f in zip(dyn.gpr_err, tdyn.gpr_err, scratch.gpr_err):
            assert torch.equal(t.X_train, f.X_train) and torch.equal(t.y_train, f.y_train) and torch.equal(g.X_train, f.X_train)
            assert torch.equal(g.y_train, f.y_train)
            assert torch.equal(t.Kf, f.Kf) and torch.equal(t.Ky, f.Ky) and torch.equal(t.Ky_inv, f.Ky_inv)
        rebuilt = dyn.gpr_err[0]._appends_since_rebuild == 0
        assert rebuilt == (before >= 8)
        if rebuilt:
            rebuilds += 1
            for g, f in zip(dyn.gpr_err, scratch.gpr_err):
                assert torch.equal(g.Ky_inv, f.Ky_inv)
            fresh = G.GPPack(scratch.gpr_err[0].X_train, torch.cat([g.y_train.reshape(-1, 1) for g in scratch.gpr_err], dim=1),
                             torch.stack([g.Ky_inv for g in scratch.gpr_err]), np.stack([g.get_lambdas() for g in scratch.gpr_err]),
                             np.array([g.get_sigma_f() for g in scratch.gpr_err]))
            r = G.rollout(fresh, z["x0"][0], z["U"][0], mpc._cost_params())
            assert c == r["cost"][0].item(), k
        else:
            gp = O.GPBundle(Xw, Yw, np.stack([g.get_lambdas() for g in dyn.gpr_err]), [g.get_sigma_f() for g in dyn.gpr_err],
                            [g.get_sigma_n() for g in dyn.gpr_err])
            means, covs = O.forward_propagate(gp, H, z["x0"][0], torch.as_tensor(z["U"][0]))
            r = dyn.rollout(z["x0"][0], z["U"][0])
            m_o = torch.stack(means).numpy()
            v_o = torch.stack([torch.diagonal(cv) for cv in covs]).numpy()
            m_g, v_g = r["means"][0].cpu().numpy(), r["vars"][0].cpu().numpy()
            worst_m = max(worst_m, float(np.abs(m_g - m_o).max() / np.abs(m_o).max()))
            worst_v = max(worst_v, float(np.abs(v_g[1:] / v_o[1:] - 1).max()))
            np.testing.assert_allclose(m_g, m_o, rtol=1e-5, atol=1e-9)
            np.testing.assert_allclose(v_g, v_o, rtol=1e-4, atol=1e-12)
    print("  %d rebuild steps; others against the oracle: means %.3e, variances %.3e (relative)" % (rebuilds, worst_m, worst_v))
    assert rebuilds == 30 // 9
    assert lib().gpmpc_pack_callback_captures(p0.handle) == captures_after_first   # no capture after the first windowed step


def test_window_bulk_call_keeps_the_newest_rows_in_chronological_order(G):
    """A bulk call into a (partly rotated) full window: the newest max_train rows, oldest first, a rebuild, slot 0."""
    rng = np.random.default_rng(8)
    dyn = G.Dynamics(2, 1)
    for gp in dyn.gpr_err:
        gp.set_lambdas(np.array([1.0, 2.0, 3.0])); gp.set_sigma_n(np.array(1e-1))
    f = lambda S: S + 0.1 * np.tanh(S)  # noqa: E731
    S, A = rng.uniform(-1, 1, (20, 2)), rng.uniform(-1, 1, (20, 1))
    dyn.max_train = 12
    dyn.append_train_data(S[:8], A[:8], f(S[:8]))                          # below the budget: appended as ever
    dyn.append_train_data(S[8], A[8], f(S[8]), incremental=True)
    assert dyn.gpr_err[0].num_train == 9 and dyn.window_slot == 0
    dyn.append_train_data(S[9:14], A[9:14], f(S[9:14]))                    # 14 rows arrive in all: rows 2..13 stay
    chron = list(range(2, 14))
    np.testing.assert_array_equal(dyn.gpr_err[0].X_train.cpu().numpy(), np.concatenate((S, A), axis=1)[chron])
    for k in (14, 15, 16):                                                # three windowed steps: slots 0, 1, 2
        dyn.append_train_data(S[k], A[k], f(S[k]), incremental=True)
    assert dyn.window_slot == 3
    dyn.append_train_data(S[17:19], A[17:19], f(S[17:19]))                 # bulk into the rotated window
    chron = list(range(7, 19))
    assert dyn.window_slot == 0 and all(g.num_train == 12 for g in dyn.gpr_err)
    for a, g in enumerate(dyn.gpr_err):
        np.testing.assert_array_equal(g.X_train.cpu().numpy(), np.concatenate((S, A), axis=1)[chron])
        np.testing.assert_array_equal(g.y_train.cpu().numpy().reshape(-1), f(S)[chron, a])
        ref = G.GaussianProcessRegression(3)
        ref.set_lambdas(np.array([1.0, 2.0, 3.0])); ref.set_sigma_n(np.array(1e-1))
        ref.append_train_data(np.concatenate((S, A), axis=1)[chron], f(S)[chron, a])
        assert torch.equal(g.Ky, ref.Ky)
        np.testing.assert_allclose(g.Ky_inv.cpu().numpy(), ref.Ky_inv.cpu().numpy(), rtol=0, atol=1e-12 * float(ref.Ky_inv.abs().max()))
    assert dyn.pack().N == 12


def test_windowed_closed_loop(G):
    """The set-up of test_closed_loop_simulator with a window of the 40 pre-training rows: 90 steps, every slot replaced at least
    twice, the training set and the pack stay where they were."""
    from gaussian_process_mpc_amd._lib import lib
    rng = np.random.default_rng(3)
    plant = G.PendulumPlant(init_state=(0.3, 0.0))
    S = np.stack((rng.uniform(-1, 1, 40), rng.uniform(-2, 2, 40)), axis=1)
    A = rng.uniform(-2, 2, (40, 1))
    nxt = np.array([G.PendulumPlant(init_state=s).step(a)[0] for s, a in zip(S, A)])
    mpc = G.RiskSensitiveMPC(-1.0, 5, 2, 1, 0.5 * np.eye(2), 0.01 * np.eye(1))
    for g in mpc.dynamics.gpr_err:
        g.set_lambdas(np.array([1.0, 4.0, 4.0]))
        g.set_sigma_n(np.array(1e-2))
    mpc.dynamics.append_train_data(S, A, nxt)
    mpc.set_lb([-2.0]); mpc.set_ub([2.0])
    p0 = mpc.dynamics.pack()
    X0 = mpc.dynamics.gpr_err[0].X_train.clone()
    sim = G.Simulator(mpc, plant, num_iters=90, incremental=True, refresh="newton", max_train=40)
    assert mpc.dynamics.max_train == 40
    hist = sim.run()
    assert len(hist) == 90 and hist[0][1].shape == (1,)
    assert 90 // 40 >= 2 and mpc.dynamics.window_slot == 90 % 40            # 90 replacements: every slot at least twice
    assert all(g.num_train == 40 for g in mpc.dynamics.gpr_err)
    assert mpc.dynamics.pack() is p0 and p0.N == 40
    Xe = mpc.dynamics.gpr_err[0].X_train
    assert Xe.shape == (40, 3) and not (Xe == X0).all(dim=1).any()          # no pre-training row is left
    # slot order: the last observation (history entry 89) sits in slot 9, the one before in slot 8
    np.testing.assert_array_equal(Xe[9].cpu().numpy(), np.concatenate((hist[89][0], hist[89][1])))
    np.testing.assert_array_equal(Xe[8].cpu().numpy(), np.concatenate((hist[88][0], hist[88][1])))
    assert all(np.isfinite(h[2]) for h in hist) and all(abs(h[1][0]) <= 2.0 + 1e-9 for h in hist)
    # horizon, flags and cost never changed and the pack was refilled in place: ONE capture of the callback graph in 90 steps
    assert lib().gpmpc_pack_callback_captures(p0.handle) == 1
