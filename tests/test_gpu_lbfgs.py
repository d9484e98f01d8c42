"""GPU tests of the device L-BFGS search: k_lbfgs_start / k_lbfgs_tick / k_lbfgs_finish (csrc/lbfgs.hip) against the numpy restatement of
tests/lbfgs_reference.py on hand-made states, batch independence, gpmpc_lbfgs_solve against its parts, the search on c1, and solver="lbfgs" of
RiskSensitiveMPC open and closed loop.

Tolerance of the tick parity (test 1): not chosen in advance.  The restatement is evaluated on the same inputs in float64 and in np.longdouble
on the CPU; the tolerance of a floating-point field is 8 x the largest relative difference seen between the two (over all fields of the case,
each difference relative to the largest magnitude of its field), scaled by the largest magnitude of that field, with a floor of 1e-13.  The
factor 8 covers the kernel's different but fixed summation order.  Flags, cnt, iters and the not-done counter are compared exactly, and every
inequality of the rule that compares computed quantities is asserted to have a relative margin of at least 1e-6 on the inputs used, so that no
decision hinges on rounding.  Measured on an MI355X over the 36 cases: the largest float64-against-longdouble relative difference is 8.9e-16
(8 x that is 7.1e-15 relative: the floor of 1e-13 is what holds for every field of magnitude below 14), the largest device-against-restatement difference 8.9e-16
relative, the smallest margin of an inequality 4.7e-5."""
import ctypes

import numpy as np
import pytest
import torch

import lbfgs_reference as R
from nominal_reference import synth_nominal

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
ZERO_PLAN_COST = 2.375489                                    # c1 from the zero start
OPT = dict(gtol=1e-4, ftol=1e-3, c1=1e-4, min_step=1e-12)   # of the hand-made states: ftol large enough for a margin on its inequality
FLOAT_FIELDS = ("X", "F", "G", "D", "A", "XT")
SCENARIOS = ("accept", "reject_pair", "shrink", "stall", "gtol", "ftol", "nan_f", "nan_g", "pinned", "reset", "wrapped", "done", "inf_f", "inf_g")


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    return g


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)).view(np.uint64)


def _shape(n):
    return {1: (1, 1), 3: (1, 3), 20: (10, 2), 64: (64, 1), 65: (13, 5), 130: (65, 2)}[n]          # (H, da)


# ------------------------------------------------------------------------------------------------------------------------------
# hand-made states
# ------------------------------------------------------------------------------------------------------------------------------
def _hand_made(K, n, m, seed):
    """K states and the evaluation (ft, gt) of their trial points, start k built for SCENARIOS[(k + seed) % len]: the box is [-1, 1]."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.6, 0.6, (K, n))
    G = rng.uniform(0.5, 1.5, (K, n)) * rng.choice([-1.0, 1.0], (K, n))
    F = rng.uniform(1.0, 2.0, K)
    D = -G * rng.uniform(0.5, 1.0, (K, 1))
    A = np.full(K, 0.25)
    cnt = rng.integers(0, m + 1, K)
    S = rng.uniform(0.05, 0.2, (K, m, n)) * rng.choice([-1.0, 1.0], (K, m, n))
    Y = S * rng.uniform(0.5, 2.0, (K, m, n))                 # positive curvature along every pair
    head = np.arange(K) % m
    done = np.zeros(K, dtype=bool)
    kind = [SCENARIOS[(k + seed) % len(SCENARIOS)] for k in range(K)]
    for k, sc in enumerate(kind):
        if sc == "stall":
            A[k] = 1e-12                                     # A / 2 max|D| <= 0.75e-12 < min_step
        if sc == "ftol":
            A[k] = 1e-3                                      # a short step: the Armijo bound is F - O(1e-7 n)
        if sc == "pinned":
            A[k] = 1.0
            D[k, : (n + 1) // 2] = np.where(np.arange((n + 1) // 2) % 2 == 0, 3.0, -3.0)      # the trial point is clipped onto both bounds
            D[k, (n + 1) // 2:] *= 0.2                       # (the other half stays inside the box)
        if sc == "reset":
            cnt[k] = 1
            Y[k, 0] = -2.0 * S[k, 0]                         # the one stored pair has negative curvature: H is negative definite
        if sc == "wrapped":
            cnt[k] = m
        if sc == "done":
            done[k] = True
    rho = 1.0 / np.einsum("kmn,kmn->km", S, Y)
    XT = np.clip(X + A[:, None] * D, -1.0, 1.0)
    XT[done] = X[done]
    step = XT - X
    ft, gt = F - 0.3, G + step * rng.uniform(0.5, 2.0, (K, n))         # default: accept, the new pair has positive curvature
    for k, sc in enumerate(kind):
        if sc in ("reject_pair", "reset"):
            gt[k] = G[k] - step[k] * rng.uniform(0.5, 2.0, n)          # s.y < 0: the pair is not stored
        if sc in ("shrink", "stall"):
            ft[k] = F[k] + 1.0
        if sc == "gtol":
            gt[k] = 1e-6 * rng.uniform(-1, 1, n)
        if sc == "ftol":
            ft[k] = F[k] - 1e-4
        if sc == "nan_f":
            ft[k] = NAN
        if sc == "inf_f":
            ft[k] = -INF
        if sc == "nan_g":
            gt[k, n // 2] = NAN
        if sc == "inf_g":
            gt[k, n - 1] = INF
        if sc == "pinned":
            at_ub, at_lb = XT[k] == 1.0, XT[k] == -1.0
            gt[k] = np.where(at_ub, -np.abs(gt[k]), np.where(at_lb, np.abs(gt[k]), gt[k]))
        if sc == "done":
            ft[k], gt[k] = -5.0, rng.uniform(-1, 1, n)       # a tempting evaluation: it must be ignored
    st = {"X": X, "F": F, "G": G, "D": D, "A": A, "XT": XT, "S": S, "Y": Y, "rho": rho, "cnt": cnt.astype(np.int64),
          "iters": rng.integers(0, 9, K).astype(np.int64), "alive": np.ones(K, dtype=bool), "done": done, "converged": done.copy()}
    return st, head, ft, gt, kind


def _device_tick(st, head, ft, gt, H, da):
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_state_fields, lbfgs_state_from_fields, lbfgs_tick
    K, m, _ = st["S"].shape
    before = lbfgs_state_from_fields({**st, "head": head}, H, da)
    after = lbfgs_tick(before.clone(), ft, gt.reshape(K, H, da), K, H, da, lb=-1.0, ub=1.0, history=m, **OPT)
    return before, after, lbfgs_state_fields(after, K, H, da, m)


def _margin(lhs, rhs, scale=None):
    """Relative distance of the two sides of an inequality (NaN entries: the inequality was not evaluated)."""
    lhs, rhs = np.asarray(lhs, dtype=np.float64), np.asarray(rhs, dtype=np.float64)
    scale = np.maximum(np.abs(lhs), np.abs(rhs)) if scale is None else scale
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(lhs - rhs) / scale
    return r[np.isfinite(r)]


def _assert_margins(rep, K):
    worst = INF
    a, b = rep["armijo"]
    checks = [_margin(a, b)]
    if "pair" in rep:
        _, sy, thr, _ = rep["pair"]
        checks.append(_margin(sy, thr))
        _, gain, bound = rep["small"]
        checks.append(_margin(gain, bound))
        _, slope, mass = rep["slope"]
        checks.append(_margin(slope, 0.0, np.where(mass > 0, mass, NAN)))       # slope < 0, relative to sum |d_c g_c|
        _, pg = rep["pg"]
        checks.append(_margin(pg, OPT["gtol"]))
    if "stall" in rep:
        checks.append(_margin(rep["stall"][1], OPT["min_step"]))
    for c in checks:
        if len(c):
            worst = min(worst, c.min())
    assert worst >= 1e-6, worst
    return worst


@pytest.mark.parametrize("m", [1, 8])
@pytest.mark.parametrize("n", [1, 3, 20, 64, 65, 130])
@pytest.mark.parametrize("K", [1, 5, 64])
def test_tick_matches_the_restatement(G, K, n, m):
    """One tick of hand-made states against the restatement.  Measured on an MI355X over the 36 cases (each case prints its own figures):
    float64 against longdouble at most 8.9e-16 relative (K = 5, n = 130, m = 1), so the tolerance is the floor of 1e-13 but for the
    fields of large magnitude (rho); device against restatement at most 8.9e-16 relative (K = 64, n = 130, m = 8)."""
    H, da = _shape(n)
    seed = 1000 * m + 10 * n + K
    st, head, ft, gt, kind = _hand_made(K, n, m, seed)
    ref, rep = R.tick(st, ft, gt, -1.0, 1.0, want_report=True, **OPT)
    ld = lambda a: np.asarray(a, dtype=np.longdouble) if np.asarray(a).dtype == np.float64 else a       # noqa: E731
    ref_ld = R.tick({k: ld(v) for k, v in st.items()}, ld(ft), ld(gt), np.longdouble(-1.0), np.longdouble(1.0), **OPT)
    worst_margin = _assert_margins(rep, K)
    # the branches: what was built is what the restatement took
    expect = {"accept": "accept+pair", "reject_pair": "accept-pair", "shrink": "shrink", "stall": "stall", "gtol": "accept+pair+gtol",
              "ftol": "accept+pair+ftol", "nan_f": "shrink", "inf_f": "shrink", "nan_g": "shrink", "inf_g": "shrink", "reset": "accept-pair",
              "wrapped": "accept+pair", "done": "done"}
    for k, sc in enumerate(kind):
        if sc == "pinned":
            assert rep["branch"][k].startswith("accept"), (k, rep["branch"][k])
            fm = R.free_mask(ref["X"][k], ref["G"][k], -1.0, 1.0)
            assert (~fm).sum() == (n + 1) // 2 and (ref["D"][k][~fm] == 0).all()
            assert n < 4 or ((ref["X"][k] == 1.0).any() and (ref["X"][k] == -1.0).any())
        else:
            assert rep["branch"][k] == expect[sc], (k, sc, rep["branch"][k])
        if sc == "reset":
            assert rep["reset"][k] and ref["cnt"][k] == 0
        if sc == "wrapped":
            assert rep["wrapped"][k] and ref["cnt"][k] == m
        if sc in ("nan_f", "inf_f"):
            assert rep["nonfinite_f"][k]
        if sc in ("nan_g", "inf_g"):
            assert rep["nonfinite_g"][k]
    before, after, got = _device_tick(st, head, ft, gt, H, da)
    # exact fields
    for f in ("alive", "done", "converged", "cnt", "iters"):
        np.testing.assert_array_equal(got[f], ref[f], err_msg=f)
    best, f_best, not_done = R.finish(ref)
    assert (got["not_done"], got["best"]) == (not_done, best)
    np.testing.assert_array_equal(got["ticks"], (~st["done"]).astype(np.int64))
    # floating-point fields: tolerance from the restatement's own float64-against-longdouble difference
    pairs = lambda s: np.arange(m)[None, :] < s["cnt"][:, None]          # noqa: E731
    valid = pairs(ref)
    fields = {f: (ref[f], np.asarray(ref_ld[f]), got[f]) for f in FLOAT_FIELDS if f != "XT"}
    fields["XT"] = (R.trial_points(ref), R.trial_points(ref_ld), got["XT"])        # (the batch the next evaluation reads: X where done)
    for f in ("rho", "S", "Y"):
        mask = valid if f == "rho" else valid[:, :, None]
        fields[f] = tuple(np.where(mask, a, 0.0) for a in (ref[f], np.asarray(ref_ld[f]), got[f]))
    fin = lambda a: np.where(np.isfinite(np.asarray(a, dtype=np.float64)), a, 0.0)    # noqa: E731
    rel = 0.0
    for f, (a64, ald, _) in fields.items():
        scale = np.abs(fin(a64)).max()
        if scale > 0:
            rel = max(rel, float(np.abs(fin(ald) - fin(a64).astype(np.longdouble)).max() / scale))
    worst = 0.0
    for f, (a64, _, dev) in fields.items():
        np.testing.assert_array_equal(np.isfinite(a64), np.isfinite(dev), err_msg=f)
        scale = np.abs(fin(a64)).max()
        tol = max(8.0 * rel * scale, 1e-13)
        err = float(np.abs(fin(dev) - fin(a64)).max())
        worst = max(worst, err / max(scale, 1e-300))
        assert err <= tol, (f, err, tol, rel)
    np.testing.assert_allclose(got["f_best"], f_best, rtol=0, atol=max(8.0 * rel * abs(f_best), 1e-13))
    np.testing.assert_array_equal(_bits(got["plan"]), _bits(got["X"][best]))
    print("K = %d, n = %d, m = %d: float64 vs longdouble %.2e relative, device vs restatement %.2e relative (allowed %.2e), smallest margin "
          "%.1e" % (K, n, m, rel, worst, max(8 * rel, 1e-13), worst_margin))
    # a done start is left bit for bit as it is (every field of it, the trial point included)
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_state_view
    vb, va = lbfgs_state_view(before, K, H, da, m), lbfgs_state_view(after, K, H, da, m)
    for k in np.where(st["done"])[0]:
        for f in ("F", "converged", "alive", "iters", "ticks", "done", "A", "cnt", "head", "rho", "X", "G", "D", "U", "S", "Y"):
            np.testing.assert_array_equal(_bits(va[f][k]), _bits(vb[f][k]), err_msg=f)
    # a rejected trial point touches neither X, G nor the pairs
    for k, sc in enumerate(kind):
        if sc in ("shrink", "stall", "nan_f", "inf_f", "nan_g", "inf_g"):
            for f in ("F", "X", "G", "D", "rho", "S", "Y", "cnt", "head", "iters"):
                np.testing.assert_array_equal(_bits(va[f][k]), _bits(vb[f][k]), err_msg=f)
    if K == 64:                                              # every branch of the rule is in every K = 64 case
        assert set(kind) == set(SCENARIOS)


def test_start_matches_the_restatement(G):
    """The start step on K = 7, n = 130: one start with a NaN value, one with an infinite gradient component, one converged at once, one
    clipped onto the box with pinned components."""
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_start, lbfgs_state_fields
    K, n, m = 7, 130, 4
    H, da = _shape(n)
    rng = np.random.default_rng(5)
    X0 = rng.uniform(-1.5, 1.5, (K, n))
    F, Gr = rng.uniform(1, 2, K), rng.uniform(0.5, 1.5, (K, n)) * rng.choice([-1.0, 1.0], (K, n))
    F[1] = NAN
    Gr[2, 77] = INF
    Gr[3] *= 1e-6
    X0[4] = np.where(np.arange(n) % 2 == 0, 4.0, -4.0)
    Gr[4] = np.where(np.arange(n) % 4 < 2, -1.0, 1.0) * np.abs(Gr[4])       # half of the components pinned
    ref = R.start(X0, F, Gr, -1.0, 1.0, m, gtol=1e-4)
    state, x0b = lbfgs_start(X0.reshape(K, H, da), F, Gr.reshape(K, H, da), lb=-1.0, ub=1.0, history=m, x0=np.array([0.5, -0.25, 2.0]))
    got = lbfgs_state_fields(state, K, H, da, m)
    np.testing.assert_array_equal(x0b.cpu().numpy(), np.tile([0.5, -0.25, 2.0], (K, 1)))
    for f in ("alive", "done", "converged", "cnt", "iters"):
        np.testing.assert_array_equal(got[f], ref[f], err_msg=f)
    assert ref["alive"].tolist() == [True, False, False, True, True, True, True] and ref["done"].tolist() == [False, True, True, True] + [False] * 3
    for f in ("X", "F", "G"):                                # copies, clips and selects: exact
        np.testing.assert_array_equal(_bits(got[f]), _bits(ref[f]), err_msg=f)
    np.testing.assert_array_equal(_bits(got["D"]), _bits(ref["D"]))          # -g_free: exact
    np.testing.assert_allclose(got["A"], ref["A"], rtol=2e-14)               # 1 / |g|_2: n = 130 squares summed in another order, n 2^-53
    np.testing.assert_allclose(got["XT"], R.trial_points(ref), rtol=0, atol=1e-14)
    assert not got["S"].any() and not got["Y"].any() and not got["rho"].any()
    assert (got["not_done"], got["best"]) == R.finish(ref)[2:] + R.finish(ref)[:1]
    # without an evaluation: only the batch of the start evaluation
    only = lbfgs_start(X0.reshape(K, H, da), lb=-1.0, ub=1.0, history=m)
    v = lbfgs_state_fields(only, K, H, da, m)
    np.testing.assert_array_equal(_bits(v["XT"]), _bits(np.clip(X0, -1.0, 1.0)))
    assert not v["X"].any() and not v["F"].any()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. batch independence
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(20, 8), (130, 3)])
def test_batch_independence_and_reproducibility(G, n, m):
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_state_view
    K = 64
    H, da = _shape(n)
    st, head, ft, gt, kind = _hand_made(K, n, m, 7)
    _, a, _ = _device_tick(st, head, ft, gt, H, da)
    _, b, _ = _device_tick(st, head, ft, gt, H, da)
    np.testing.assert_array_equal(_bits(a), _bits(b))        # two identical calls: the whole buffer
    va = lbfgs_state_view(a, K, H, da, m)
    for k in range(K):
        one = {f: (v[k:k + 1] if isinstance(v, np.ndarray) else v) for f, v in st.items()}
        _, s1, _ = _device_tick(one, head[k:k + 1], ft[k:k + 1], gt[k:k + 1], H, da)
        v1 = lbfgs_state_view(s1, 1, H, da, m)
        for f in ("F", "converged", "alive", "iters", "ticks", "done", "A", "cnt", "head", "rho", "X", "G", "D", "U", "S", "Y"):
            np.testing.assert_array_equal(_bits(v1[f][0]), _bits(va[f][k]), err_msg="%s of start %d (%s)" % (f, k, kind[k]))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. / 4. on c1
# ------------------------------------------------------------------------------------------------------------------------------
_c1 = {}


def _problem(G):
    if not _c1:
        from gaussian_process_mpc_amd.multistart import make_starts
        from gaussian_process_mpc_amd.synth import synth_problem
        from oracle import gpmpc_oracle as O
        pb = synth_problem(1, 100, 2, 2, 10, 64)
        gp = O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"])
        n = pb["H"] * pb["da"]
        X0 = make_starts(4, n, np.full(n, -1.0), np.full(n, 1.0), np.random.default_rng([0, 0]))
        _c1.update(pb=pb, gp=gp, X0=X0)
    return _c1["pb"], _c1["gp"], _c1["X0"]


def _pack(G, nominal=False):
    pb, gp, _ = _problem(G)
    return G.GPPack(pb["X"], pb["Y"], gp.Ky_inv.numpy(), pb["lambdas"], pb["sigma_f"], nominal=synth_nominal(2, 2) if nominal else None)


def _cost(G):
    pb = _problem(G)[0]
    return G.CostParams(1e-5, pb["Q"], pb["R"], x_ref=pb["x_ref"], u_ref=pb["u_ref"])


def _last_state(log):
    def callback(ticks, ws):
        log.append((ticks, ws.clone()))
    return callback


def test_solve_equals_its_parts_bit_for_bit(G):
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_solve, lbfgs_start, lbfgs_state_layout, lbfgs_state_view, lbfgs_tick
    pb, _, X0 = _problem(G)
    pack, cost = _pack(G), _cost(G)
    H, da, x0, K, m, T = pb["H"], pb["da"], pb["x0"][0], 4, 8, 6
    total = lbfgs_state_layout(K, H * da, m)["total"]
    kw = dict(lb=-1.0, ub=1.0, history=m, gtol=1e-4, ftol=1e-10)
    one, two = [], []
    U1, c1, info1 = lbfgs_solve(pack, x0, X0.reshape(K, H, da), cost, max_ticks=T, check_every=0, callback=_last_state(one), **kw)
    U2, c2, info2 = lbfgs_solve(pack, x0, X0.reshape(K, H, da), cost, max_ticks=T, check_every=T // 2, callback=_last_state(two), **kw)
    assert [t for t, _ in one] == [T] and [t for t, _ in two] == [T // 2, T]
    np.testing.assert_array_equal(_bits(one[-1][1][:total]), _bits(two[-1][1][:total]))         # one chunk of T = two chunks of T / 2
    np.testing.assert_array_equal(_bits(U1), _bits(U2))
    # the parts: start evaluation, start step, T x (rollout, tick) through the pure entries
    Xd = torch.as_tensor(X0.reshape(K, H, da), device="cuda")
    state = lbfgs_start(Xd, **kw)
    v = lbfgs_state_view(state, K, H, da, m)
    r = G.rollout(pack, x0, v["U"], cost, want_grad=True, want_traj=False)
    lbfgs_start(Xd, r["cost"], r["grad"], state=state, **kw)
    for _ in range(T):
        r = G.rollout(pack, x0, v["U"], cost, want_grad=True, want_traj=False)
        lbfgs_tick(state, r["cost"], r["grad"], K, H, da, **kw)
    np.testing.assert_array_equal(_bits(state[:total]), _bits(one[-1][1][:total]))
    assert c1 == float(state[2].item()) and info1["best"] == int(state[1].item()) and info1["ticks"] == T and info1["evaluations"] == T + 1
    np.testing.assert_array_equal(_bits(U1), _bits(v["plan"]))


def test_it_solves(G):
    """c1, K = 4, row 0 the zero start, gtol = 1e-4; ftol = 0 and min_step = 0, so that a start reported converged converged by gtol."""
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_solve, lbfgs_state_fields, lbfgs_state_layout
    from oracle import gpmpc_oracle as O
    pb, gp, X0 = _problem(G)
    pack, cost = _pack(G), _cost(G)
    H, da, x0, K, m = pb["H"], pb["da"], pb["x0"][0], 4, 8
    n = H * da
    assert not X0[0].any()
    kw = dict(lb=-1.0, ub=1.0, history=m, gtol=1e-4, ftol=0.0, min_step=0.0)
    log = []
    U, best_cost, info = lbfgs_solve(pack, x0, X0.reshape(K, H, da), cost, max_ticks=150, check_every=1, callback=_last_state(log), **kw)
    total = lbfgs_state_layout(K, n, m)["total"]
    states = [lbfgs_state_fields(ws[:total], K, H, da, m) for _, ws in log]
    Fs = np.array([s["F"] for s in states])
    print("ticks %d, F %s, converged %s, iterations %s" % (info["ticks"], info["f"], info["converged"], info["iterations"]))
    assert np.all(Fs[1:] <= Fs[:-1])                         # every start's F is non-increasing over the ticks
    assert best_cost <= ZERO_PLAN_COST and best_cost == info["f"][info["best"]] == info["f"].min() and np.all(np.abs(U) <= 1.0)
    np.testing.assert_array_equal(_bits(U.reshape(-1)), _bits(info["x"][info["best"]]))
    # converged starts: max |g_free| <= gtol by an independent rollout call
    assert info["converged"].any()
    r = G.rollout(pack, x0, info["x"].reshape(K, H, da), cost, want_grad=True, want_traj=False)
    g = r["grad"].cpu().numpy().reshape(K, n)
    pg = np.abs(np.where(R.free_mask(info["x"], g, -1.0, 1.0), g, 0.0)).max(axis=1)
    print("max |g_free| of every start:", pg)
    assert np.all(pg[info["converged"]] <= 1e-4)
    np.testing.assert_allclose(r["cost"].cpu().numpy(), info["f"], rtol=1e-12)
    # row 0 against the restatement driven by the same device rollouts
    def evaluate(X):
        rr = G.rollout(pack, x0, X.reshape(-1, H, da), cost, want_grad=True, want_traj=False)
        return rr["cost"].cpu().numpy(), rr["grad"].cpu().numpy().reshape(-1, n)
    trace = []
    _, ref = R.solve(evaluate, X0, np.full(n, -1.0), np.full(n, 1.0), max_ticks=150, trace=trace, **{k: v for k, v in kw.items() if k not in ("lb", "ub")})
    seq_ref = [row[0].split("+")[0].split("-")[0] for row in trace]
    seq_dev, iters_prev, done_prev = [], 0, False            # (the zero start is not done by its first gradient)
    for s in states:                                         # states[t]: after tick t + 1
        seq_dev.append("done" if done_prev else ("accept" if s["iters"][0] > iters_prev else "shrink"))
        iters_prev, done_prev = s["iters"][0], bool(s["done"][0])
    seq_ref = [b if b != "stall" else "shrink" for b in seq_ref]
    k = min(len(seq_ref), len(seq_dev))
    assert seq_dev[:k] == seq_ref[:k] and all(b == "done" for b in seq_dev[k:] + seq_ref[k:]), (seq_dev, seq_ref)
    # ... for which that sequence is stable: the restatement on oracle evaluations perturbed by +-1e-12 relative takes the same decisions
    def oracle(sign):
        prng = np.random.default_rng(11)
        def ev(X):
            f, gg = [], []
            for u in X:
                o = O.objective_and_gradient(gp, H, x0, u.reshape(H, da), pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], 1e-5)
                f.append(o["cost"])
                gg.append(np.asarray(o["grad"]).reshape(-1))
            f, gg = np.array(f), np.array(gg)
            return f * (1 + sign * 1e-12), gg * (1 + sign * 1e-12 * prng.choice([-1.0, 1.0], gg.shape))
        return ev
    seqs = []
    for sign in (0.0, 1.0, -1.0):
        tr = []
        R.solve(oracle(sign), X0[:1], np.full(n, -1.0), np.full(n, 1.0), max_ticks=len(seq_ref), trace=tr,
                **{k: v for k, v in kw.items() if k not in ("lb", "ub")})
        seqs.append([row[0].split("+")[0].split("-")[0].replace("stall", "shrink") for row in tr])
    assert seqs[0] == seqs[1] == seqs[2], seqs
    print("row 0 on the oracle:", "".join(b[0] for b in seqs[0]), "on the device:", "".join(b[0] for b in seq_dev))
    err = np.abs(info["x"][0] - ref["x"][0]).max()
    print("row 0: %d ticks, |X_device - X_restatement| = %.3e" % (len(seq_ref), err))
    assert err <= 1e-9
    assert states[-1]["iters"][0] == ref["iterations"][0]


# ------------------------------------------------------------------------------------------------------------------------------
# 5. interface and edge cases
# ------------------------------------------------------------------------------------------------------------------------------
def _mpc_c1(G):
    pb = _problem(G)[0]
    ds, da, H = pb["ds"], pb["da"], pb["H"]
    mpc = G.RiskSensitiveMPC(1e-5, H, ds, da, pb["Q"], pb["R"])
    for a, g in enumerate(mpc.dynamics.gpr_err):
        g.set_lambdas(pb["lambdas"][a])
        g.set_sigma_n(float(pb["sigma_n"][a]))
        g.set_sigma_f(1.0)
    mpc.dynamics.append_train_data(pb["X"][:, :ds], pb["X"][:, ds:], pb["Y"])
    mpc.set_lb([-1.0] * da)
    mpc.set_ub([1.0] * da)
    return mpc, pb


def test_mpc_interface_and_default_unchanged(G):
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_solve
    from gaussian_process_mpc_amd.multistart import make_starts
    mpc, pb = _mpc_c1(G)
    x0, H, da = pb["x0"][0], pb["H"], pb["da"]
    n = H * da
    assert mpc.solver is None
    before = mpc.get_optimal_trajectory(x0).copy()
    used = mpc.solver_used
    mpc.solver_used, mpc._solve_count = None, 0              # (as a fresh object: no warm start, first seed)
    mpc.n_starts = 4
    mpc.multistart_options.update(max_ticks=40, check_every=4)
    plan = mpc.get_optimal_trajectory(x0, solver="lbfgs")
    info = mpc.last_solve_info
    assert plan.shape == (H, da) and mpc.solver_used == "device-lbfgs x4" and np.all(np.abs(plan) <= 1.0)
    assert {"f", "x", "ticks", "evaluations", "converged", "alive", "best", "iterations", "starts", "sharded_over"} <= set(info)
    assert info["f"].shape == (4,) and info["x"].shape == (4, n) and info["starts"] == 4 and info["alive"].all()
    assert info["f"][info["best"]] <= ZERO_PLAN_COST and info["ticks"] <= 40
    np.testing.assert_array_equal(mpc.last_traj, plan.reshape(-1))
    # the starts, the seed and the solve count are those of the host search
    X0 = make_starts(4, n, H * [-1.0] * da, H * [1.0] * da, np.random.default_rng([0, 0]), warm=None, spread=1.0)
    U, _, _ = lbfgs_solve(mpc.dynamics.pack(), x0, X0.reshape(4, H, da), mpc._cost_params(), lb=-1.0, ub=1.0, max_ticks=40, history=6,
                          check_every=4)
    np.testing.assert_array_equal(_bits(U), _bits(plan))
    # the attribute, one start, and the second solve's warm start
    mpc.solver, mpc.n_starts = "lbfgs", 1
    plan1 = mpc.get_optimal_trajectory(x0)
    assert mpc.solver_used == "device-lbfgs x1" and plan1.shape == (H, da) and mpc.last_solve_info["f"].shape == (1,)
    with pytest.raises(ValueError, match="solver"):
        mpc.get_optimal_trajectory(x0, solver="cma")
    mpc.set_state_constraints([[1.0, 0.0]], [0.5], prob=0.95)
    with pytest.raises(NotImplementedError, match="state constraints"):
        mpc.get_optimal_trajectory(x0)
    mpc.clear_state_constraints()
    # the default solver is what it was: the same call after setting and unsetting solver
    mpc.solver, mpc.n_starts = None, 1
    after = mpc.get_optimal_trajectory(x0)
    assert mpc.solver_used == used
    np.testing.assert_array_equal(_bits(after), _bits(before))


def test_nominal_pack_and_seeds(G):
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_solve
    pb, _, X0 = _problem(G)
    H, da, x0 = pb["H"], pb["da"], pb["x0"][1]
    cost = _cost(G)
    nom, plain = _pack(G, nominal=True), _pack(G)
    kw = dict(lb=-1.0, ub=1.0, max_ticks=12, check_every=0)
    c0 = G.rollout(nom, x0, np.clip(X0, -1, 1).reshape(4, H, da), cost, want_grad=True, want_traj=False)["cost"].cpu().numpy()
    Ua, ca, ia = lbfgs_solve(nom, x0, X0.reshape(4, H, da), cost, **kw)
    Ub, cb, ib = lbfgs_solve(nom, x0, X0.reshape(4, H, da), cost, **kw)
    np.testing.assert_array_equal(_bits(Ua), _bits(Ub))
    np.testing.assert_array_equal(_bits(ia["f"]), _bits(ib["f"]))
    print("nominal pack: starts %s -> %s" % (c0, ia["f"]))
    assert np.all(ia["f"] <= c0) and ca == ia["f"].min()
    _, cp, _ = lbfgs_solve(plain, x0, X0.reshape(4, H, da), cost, **kw)
    assert cp != ca                                          # (the model changes the problem)


def test_refusals_and_error_codes(G):
    from gaussian_process_mpc_amd import _lib
    from gaussian_process_mpc_amd.device_lbfgs import lbfgs_params, lbfgs_solve, lbfgs_start, lbfgs_tick
    pb, _, X0 = _problem(G)
    H, da, x0 = pb["H"], pb["da"], pb["x0"][0]
    pack, cost = _pack(G), _cost(G)
    X = X0.reshape(4, H, da)
    good = dict(lb=-1.0, ub=1.0, max_ticks=2, check_every=0)
    for bad, text in ((dict(history=0), "history"), (dict(history=17), "history"), (dict(gtol=-1.0), "gtol"), (dict(gtol=NAN), "gtol"),
                      (dict(ftol=-1e-12), "ftol"), (dict(c1=NAN), "c1"), (dict(min_step=-1.0), "min_step"), (dict(lb=0.5, ub=0.25), r"lb\[0\]"),
                      (dict(lb=[-1.0, NAN]), r"lb\[1\]"), (dict(max_ticks=-1), "n_ticks")):
        with pytest.raises(G.GpmpcError, match="bad argument.*" + text):
            lbfgs_solve(pack, x0, X, cost, **{**good, **bad})
    with pytest.raises(G.GpmpcError, match="bad argument.*n_starts"):
        lbfgs_solve(pack, x0, np.zeros((257, H, da)), cost, **good)
    with pytest.raises(G.GpmpcError, match="bad argument.*n_starts"):
        lbfgs_start(np.zeros((257, H, da)), lb=-1.0, ub=1.0)
    with pytest.raises(G.GpmpcError, match=r"bad argument.*lb\[1\]"):
        lbfgs_start(X, lb=[-1.0, 2.0], ub=[1.0, 1.0])
    state = lbfgs_start(X, lb=-1.0, ub=1.0)
    with pytest.raises(G.GpmpcError, match="bad argument.*c1"):
        lbfgs_tick(state, np.zeros(4), np.zeros((4, H, da)), 4, H, da, c1=-1.0)
    with pytest.raises(G.GpmpcError, match="workspace too small"):
        lbfgs_tick(state[:-32], np.zeros(4), np.zeros((4, H, da)), 4, H, da)
    lib = G.lib()
    P = lbfgs_params(4, da, -1.0, 1.0)
    nbytes = lib.gpmpc_lbfgs_solve_workspace_bytes(pack.handle, H, ctypes.byref(P))
    assert nbytes > lib.gpmpc_lbfgs_state_bytes(4, H, da, 8) > 0
    buf = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    ws = torch.zeros(nbytes // 8 + 32, dtype=torch.float64, device="cuda")
    call = lambda h, nb, first=0, nt=2: lib.gpmpc_lbfgs_solve(h, H, _lib.ptr(buf[:2]), _lib.ptr(buf[64:64 + 4 * H * da]), ctypes.byref(cost.c),   # noqa: E731
                                                               ctypes.byref(P), first, nt, _lib.ptr(ws), nb, _lib.stream_ptr())
    assert call(pack.handle, nbytes - 1) == -4               # GPMPC_E_WORKSPACE
    assert call(pack.handle, nbytes, first=-1) == -1 and call(pack.handle, nbytes, nt=-1) == -1
    h = ctypes.c_void_p()                                    # a pack that is not built: GPMPC_E_STATE
    assert lib.gpmpc_pack_create(ctypes.byref(h), 100, 2, 2) == 0
    try:
        assert call(h, nbytes) == -5
    finally:
        lib.gpmpc_pack_destroy(h)
    torch.cuda.synchronize()
    assert not ws.any()                                      # nothing was launched by any of the refused calls
    assert call(pack.handle, nbytes) == 0
    torch.cuda.synchronize()
    assert ws[3].item() == 4 and ws[4].item() == H * da and ws[5].item() == 8


def test_pendulum_closed_loop_three_steps(G):
    rng = np.random.default_rng(3)
    plant = G.PendulumPlant(init_state=(0.3, 0.0))
    S = np.stack((rng.uniform(-1, 1, 100), rng.uniform(-2, 2, 100)), axis=1)
    A = rng.uniform(-2, 2, (100, 1))
    nxt = np.array([G.PendulumPlant(init_state=s).step(a)[0] for s, a in zip(S, A)])
    mpc = G.RiskSensitiveMPC(-1.0, 5, 2, 1, np.diag([10.0, 0.1]), 0.01 * np.eye(1), nominal_models=G.LinearNominalModel.identity(2, 1))
    for g in mpc.dynamics.gpr_err:
        g.set_lambdas(np.array([1.0, 4.0, 4.0]))
        g.set_sigma_n(np.array(1e-2))
    mpc.dynamics.append_train_data(S, A, nxt)
    mpc.set_lb([-2.0])
    mpc.set_ub([2.0])
    mpc.solver, mpc.n_starts = "lbfgs", 8
    log, solve = [], mpc.get_optimal_trajectory

    def logged(obs, **kw):
        plan = solve(obs, **kw)
        log.append((np.array(plan), mpc.solver_used, dict(mpc.last_solve_info)))
        return plan
    mpc.get_optimal_trajectory = logged
    hist = G.Simulator(mpc, plant, num_iters=3, incremental=True).run()
    states = np.array([h[0] for h in hist])
    assert len(log) == 3 and all(s == "device-lbfgs x8" for _, s, _ in log)
    assert np.all(np.isfinite(states)) and all(np.all(np.abs(p) <= 2.0) and np.all(np.isfinite(p)) for p, _, _ in log)
    assert all(i["alive"].all() and np.isfinite(i["f"]).all() and i["f"][i["best"]] == i["f"].min() for _, _, i in log)
    print("theta %.3f -> %.3f, ticks per solve %s" % (states[0, 0], states[-1, 0], [i["ticks"] for _, _, i in log]))
