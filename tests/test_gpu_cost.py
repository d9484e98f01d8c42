"""The COST PATH on the device -- the four hand-written eliminations (state_cost in k_cost_full, state_cost_sched<1..8> in k_cost_sched,
state_cost_diag<DS> in k_roll_tail, fc_state_cost<DS> in k_fc_tail), the three input costs and the reverse sweeps -- against the long double
restatement of tests/cost_reference.py, on inputs that make the eliminations PIVOT: gamma = -0.9 / rho(Q Sigma), coupled Q, covariances of
order one (a noise model with process_var ~ U(0.3, 3) for the rollouts), the 'tiny' family whose leading entry is 1e-6.  The inputs of the
older tests never swap a row in three of the four eliminations (tests/test_host_cost.py asserts that, with the table of defects this buys).

K = |HIP - long double| / (2^-53 A), A from the reference alone (tests/cost_reference.py).  Asserted per form and output: for every launch
K <= 10 max(K_ref, 0.5), K_ref the float64 emulation of the same elimination on the inputs of that launch (half a unit is what one correctly
rounded operation may err by: a K_ref of two or three entries that rounds to zero by luck is no sharper floor); over the launches of one
parametrised case pooled, K <= 10 K_ref; and the caps of tests/cost_reference.py::CAP_K, twice the worst K measured on an MI355X.

The fused tails are judged on the HIP path's OWN means and variances (covariances), so the GP arithmetic stays out; the gradient of
k_roll_tail against the long double sweep over the Jacobians gpmpc_rollout_jac returns for the same call plus the long double input-cost
gradient.  gpmpc_rollout_jac runs the same head kernels under the same plan: its means and variances are asserted bit-equal to the rollout's.
The derivatives of state_cost_diag and fc_state_cost and the gradient of input_cost_step are seen through the tails' gradients only; the
full-covariance gradient (R_delta and last_u included) against the long double complex step of the CPU port (oracle/cport/gpmpc_cpu_given.c
under the pack's noise model) plus the long double R_delta term, with the floor of tests/test_gpu_accuracy.py, the double complex build's own
error.  That port knows no schedule: the SCHED instances of k_fc_tail are held in value (test_fullcov_tail_cost, time-varying rows and Q_f)
and, for the gradient, to the bits of the plain instance under a schedule of constant rows; their gradient under time-varying rows or a
Q_f is held by tests/test_gpu_tracking.py at small variances only, not here.

Measured on an MI355X, worst K per form and output (K_ref of the same pooled case in brackets):
    k_cost_full                     value 2.31 (3.13)    d/dmu 3.55 (3.24)    d/dSigma 3.64 (3.64)
    k_cost_sched<1..8>              value 3.05 (1.46)    d/dmu 3.34 (3.34)    d/dSigma 4.13 (4.13)
    input_cost                      d/dU 2.93 (2.93)
    k_rollout_vjp                   gU 2.15 (2.64)       gx0 2.01 (2.05)
    k_roll_tail                     value 0.62 (0.62)    gradient: all-in-LDS sweep 0.47 (0.42), streaming sweep 0.70 (0.63)
    k_fc_tail                       value 1.14 (1.14)    complex step: cost 1.3e-14 (floor 1.4e-13), gradient 3.9e-14 (floor 4.9e-13)
No form lies more than a factor 2.1 above K_ref.  The caps (tests/cost_reference.py::CAP_K, CAP_REL) are twice these, rounded up to two digits.

Checked once on scratch copies of the kernels (not committed), each built into a library of its own and run against this module and against
the rest of the GPU suite: without `if (piv != k) det = -det;` in state_cost_diag all ten cases of test_fused_tail_cost_and_gradient with
ds >= 2 fail; with the predicated swap of state_cost_sched over the first DS columns only, test_stand_alone_cost_and_gradient fails at every
ds >= 2 and test_nan_passes_through_one_trajectory_only[sched]; without the `det = -det` of fc_state_cost's cascade, test_fullcov_tail_cost and
test_fullcov_tail_gradient_against_the_complex_step fail at every ds >= 2.  The other 701 GPU tests of the suite pass under each of the three.
"""
import ctypes

import numpy as np
import pytest
import torch

import cost_reference as C

pytestmark = pytest.mark.gpu

_WORST = {}


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    yield g
    print("\n  worst K per form and output (K_ref of the same pooled case in brackets):\n    " +
          "\n    ".join("%-28s %-8s %8.3g  (%.3g)" % (k[0], k[1], v[0], v[1]) for k, v in sorted(_WORST.items())))


def _L():
    from gaussian_process_mpc_amd._lib import lib
    return lib()


def _sp():
    from gaussian_process_mpc_amd._lib import stream_ptr
    return stream_ptr()


def _check(rc, what):
    from gaussian_process_mpc_amd._lib import check
    check(rc, what)


def _dev(a):
    """A device copy with at least one element behind it (an empty array still hands the library a pointer)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    t = torch.zeros(max(a.size, 1), dtype=torch.float64, device="cuda")
    t[:a.size] = torch.from_numpy(a.reshape(-1))
    return t


def _nan(*shape):
    return torch.full((max(int(np.prod(shape)), 1),), float("nan"), dtype=torch.float64, device="cuda")


def _np(t, *shape):
    return t[:int(np.prod(shape))].cpu().numpy().reshape(shape)


def _vp(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


class _Pool:
    """K and K_ref of the launches of one case, per (form, output); judged together at the end of the case."""

    def __init__(self):
        self.k, self.kref = {}, {}

    def add(self, form, output, k, kref):
        """One launch.  Judged at once against ITS OWN K_ref, which counts for no less than 0.5: a single correctly rounded operation errs
        by up to half a unit, so a K_ref below that over a handful of entries is luck, not a sharper floor."""
        key = (form, output)
        assert k <= 10 * max(kref, 0.5), (key, k, kref)
        self.k[key], self.kref[key] = max(self.k.get(key, 0.0), k), max(self.kref.get(key, 0.0), kref)

    def judge(self, what):
        for key, k in sorted(self.k.items()):
            kref, cap = self.kref[key], C.CAP_K[key]
            print("  %s: %s %s K %.3g (K_ref %.3g, cap %.3g)" % (what, key[0], key[1], k, kref, cap))
            if k >= _WORST.get(key, (0.0, 0.0))[0]:
                _WORST[key] = (k, kref)
        for key, k in sorted(self.k.items()):
            assert k <= 10 * self.kref[key], (what, key, k, self.kref[key])
            assert k <= C.CAP_K[key], (what, key, k, C.CAP_K[key])


def _cost_params(G, c, schedule=None):
    return G.CostParams(c["gamma"], c["Q"], c["R"].reshape(c["da"], c["da"]), R_delta=c["Rd"].reshape(c["da"], c["da"]), x_ref=c["x_ref"],
                        u_ref=c["u_ref"], last_u=c["last_u"], schedule=schedule)


def _schedule(G, c, slack=3):
    """A schedule with H < H_max: the rows of u_ref and Q_f start at offsets that depend on H_max, not on H."""
    cs = G.CostSchedule(c["H"] + slack, c["ds"], c["da"])
    cs.set(c["X_ref"], c["U_ref"] if c["da"] else None, c["Q_f"])
    return cs


def _cost_grad(G, c, schedule=None, grad=True, means=None, covs=None):
    """gpmpc_cost_grad (grad) or the value-only call with three NULL outputs, into NaN-filled buffers."""
    B, H, ds, da = c["B"], c["H"], c["ds"], c["da"]
    cp = _cost_params(G, c, schedule)
    m, s, u = _dev(c["means"] if means is None else means), _dev(c["covs"] if covs is None else covs), _dev(c["U"])
    out = _nan(B)
    dm, dc, du = (_nan(B, H + 1, ds), _nan(B, H + 1, ds, ds), _nan(B, H, da)) if grad else (None, None, None)
    _check(_L().gpmpc_cost_grad(B, H, ds, da, ctypes.byref(cp.c), _vp(m), _vp(s), _vp(u), _vp(out), _vp(dm), _vp(dc), _vp(du), _sp()),
           "gpmpc_cost_grad")
    torch.cuda.synchronize()
    r = {"cost": _np(out, B)}
    if grad:
        r.update(dmu=_np(dm, B, H + 1, ds), dsig=_np(dc, B, H + 1, ds, ds), dU=_np(du, B, H, da))
    return r


def _judge_call(pool, form, c, got, sched):
    """One stand-alone launch against the long double terms; K_ref from the float64 emulation of the same form plus the float64 input cost."""
    kw = C.call_kwargs(c)
    if not sched:
        kw.update(X_ref=None, U_ref=None, Q_f=None)
    ref = C.cost_terms(c["means"], c["covs"], c["U"], **kw)
    assert np.all(ref["det"] > 0)
    em = C.emulate_terms(form, c["means"], c["covs"], c["gamma"], c["Q"], c["x_ref"], kw["X_ref"], kw["Q_f"])
    assert em["margin"].min() >= C.TIE
    f = C.input_terms(c["U"], c["R"], c["Rd"], c["last_u"], c["u_ref"] if kw["U_ref"] is None else kw["U_ref"], dtype=np.float64)
    pool.add(form, "value", C.k_of(got["cost"], ref["value"], ref["A_value"]), C.k_of(em["value_state"].sum(1) + f["value"], ref["value"], ref["A_value"]))
    pool.add(form, "dmu", C.k_of(got["dmu"], ref["dmu"], ref["A_dmu"]), C.k_of(em["dmu"], ref["dmu"], ref["A_dmu"]))
    pool.add(form, "dsig", C.k_of(got["dsig"], ref["dsig"], ref["A_dsig"]), C.k_of(em["dsig"], ref["dsig"], ref["A_dsig"]))
    pool.add("input_cost", "dU", C.k_of(got["dU"], ref["dU"], ref["A_dU"]), C.k_of(f["dU"], ref["dU"], ref["A_dU"]))
    return em


def _stand_alone_shapes(ds):
    """(B, H, da, family, seed, q_f) of the launches per form of one state dimension: every B of the 64-thread grid edge at EVERY ds (the
    guard of each instance of k_cost_sched), H = 1, 2, 7 and da = 0, 1, 3, 8 - ds rotated with ds so that every value meets every other
    over the eight dimensions; then, at ds >= 2, the chosen draws of the 'tiny' family as two launches more (draws of the shape (2, 7, 2))."""
    Bs, Hs, das = (1, 63, 64, 65, 130), (1, 2, 7), (0, 1, 3, 8 - ds)
    fam = ("neg", "neg", "neg", "pos", "zero")
    shapes = [(Bs[i], Hs[(i + ds) % 3], das[(i + ds) % 4], fam[(i + ds) % 5], i, (i + ds) % 2 == 0) for i in range(5)]
    return shapes + [(2, 7, 2, "tiny", seed, False) for seed in (C.TINY_SEEDS[ds, False] if ds >= 2 else [])]


@pytest.mark.parametrize("ds", range(1, 9))
def test_stand_alone_cost_and_gradient(G, ds):
    """gpmpc_cost_grad: k_cost_full (no schedule) and k_cost_sched<ds> (a schedule with H < H_max, with and without Q_f; Q_f from the
    generator of Q, the slots of step H scaled under IT, so step H pivots under the terminal weight) on full non-symmetric Sigma,
    non-symmetric R and R_delta, last_u != 0.  Every entry of cost, d_means, d_covs, d_U in K; the value-only call returns the bits of the
    value of the gradient call; a constant schedule returns the bits of no schedule, on the pivoting inputs too."""
    pool, cols = _Pool(), {"full": set(), "sched": set()}
    for B, H, da, fam, seed, q_f in _stand_alone_shapes(ds):
        c = C.gen_call(seed, ds, da, H, B, fam)
        got = _cost_grad(G, c)
        cols["full"] |= C.swap_summary(_judge_call(pool, "full", c, got, False)["swaps"])[0]
        assert _same(_cost_grad(G, c, grad=False)["cost"], got["cost"])
        const = dict(c, X_ref=np.tile(c["x_ref"], (H + 1, 1)), U_ref=np.tile(c["u_ref"], (H, 1)), Q_f=None)
        cs = _schedule(G, const)
        flat = _cost_grad(G, const, schedule=cs)
        cs.close()
        assert all(_same(flat[k], got[k]) for k in got), "a constant schedule does not return the bits of no schedule"
        c = C.gen_call(seed, ds, da, H, B, fam, sched=True, q_f=q_f)
        cs = _schedule(G, c)
        got = _cost_grad(G, c, schedule=cs)
        cols["sched"] |= C.swap_summary(_judge_call(pool, "sched", c, got, True)["swaps"])[0]
        assert _same(_cost_grad(G, c, schedule=cs, grad=False)["cost"], got["cost"])
        cs.close()
    if ds >= 2:
        assert cols["full"] and cols["sched"], "no launch of this dimension swapped a row"
    pool.judge("stand-alone ds %d (columns swapped: full %s, sched %s)" % (ds, sorted(cols["full"]), sorted(cols["sched"])))


@pytest.mark.parametrize("form", ["full", "sched"])
def test_nan_passes_through_one_trajectory_only(G, form):
    """Three trajectories of 65 carry one step with gamma rho = -1.5 and a determinant below -1e-3 in the reference: their cost is NaN, every
    other trajectory stays within budget, and no output of another trajectory changes a bit against the same launch without them."""
    ds, da, H, B = 4, 2, 3, 65
    c = C.gen_call(11, ds, da, H, B, "neg", sched=form == "sched")
    cs = _schedule(G, c) if form == "sched" else None
    bad = {3: 0, 40: 2, 64: 3}
    covs = c["covs"].copy()
    for b, i in bad.items():
        rho = C.spectral_radius(c["Q"][None], covs[b, i][None])[0]
        covs[b, i] *= 1.5 / (abs(c["gamma"]) * rho)
    kw = C.call_kwargs(c)
    if form != "sched":
        kw.update(X_ref=None, U_ref=None, Q_f=None)
    ref = C.cost_terms(c["means"], covs, c["U"], **kw)
    for b, i in bad.items():
        assert ref["det"][b, i] < -1e-3 and np.isnan(ref["value"][b])
    clean, with_bad = _cost_grad(G, c, schedule=cs), _cost_grad(G, c, schedule=cs, covs=covs)
    others = np.array([b for b in range(B) if b not in bad])
    assert np.all(np.isnan(with_bad["cost"][list(bad)])) and np.all(np.isfinite(with_bad["cost"][others]))
    for k in clean:
        assert _same(clean[k][others], with_bad[k][others]), k
        if k in ("dmu", "dsig"):                              # within a poisoned trajectory the other steps are untouched too
            for b, i in bad.items():
                keep = [j for j in range(H + 1) if j != i]
                assert _same(clean[k][b, keep], with_bad[k][b, keep]), k
    pool = _Pool()
    _judge_call(pool, form, c, clean, form == "sched")
    pool.judge("the launch without the poisoned steps, %s" % form)
    if cs is not None:
        cs.close()


@pytest.mark.parametrize("ds", range(1, 9))
def test_rollout_vjp_on_random_jacobians(G, ds):
    """gpmpc_rollout_vjp (k_rollout_vjp) for da = 1 ... 8, H = 1, 2, 9, B = 1, 3: both seeds, g_means NULL, g_vars NULL, out_gx0 NULL and
    not, against the long double sweep; buffers pre-filled with NaN, so a store the kernel misses shows."""
    pool = _Pool()
    for da in range(1, 9):
        for v, (gm_on, gv_on, gx_on) in enumerate(((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0))):
            H, B = (1, 2, 9)[(ds + da + v) % 3], (1, 3)[(ds + da + v // 2) % 2]
            p = C.gen_vjp(v, ds, da, H, B)
            gm, gv = p["gm"] if gm_on else None, p["gv"] if gv_on else None
            J, out_gU, out_gx0 = _dev(p["J"]), _nan(B, H, da), _nan(B, ds) if gx_on else None
            gmd, gvd = None if gm is None else _dev(gm), None if gv is None else _dev(gv)
            _check(_L().gpmpc_rollout_vjp(B, H, ds, da, _vp(J), _vp(gmd), _vp(gvd), _vp(out_gU), _vp(out_gx0), _sp()), "gpmpc_rollout_vjp")
            torch.cuda.synchronize()
            (gU, gx0), (aU, ax0) = C.sweep(p["J"], gm, gv), C.sweep_unit(p["J"], gm, gv)
            fU, fx0 = C.sweep(p["J"], gm, gv, dtype=np.float64)
            pool.add("k_rollout_vjp", "gU", C.k_of(_np(out_gU, B, H, da), gU, aU), C.k_of(fU, gU, aU))
            if gx_on:
                pool.add("k_rollout_vjp", "gx0", C.k_of(_np(out_gx0, B, ds), gx0, ax0), C.k_of(fx0, gx0, ax0))
    pool.judge("rollout_vjp ds %d" % ds)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fused tails
# ---------------------------------------------------------------------------------------------------------------------------------------
def _problem(seed, N, ds, da, H, B, nominal=False):
    """A small GP problem of the package's generator with a noise model of order one: process_var ~ U(0.3, 3), a full init_cov."""
    from gaussian_process_mpc_amd.synth import synth_problem
    pb = synth_problem(seed, N, ds, da, H, B)
    rng = np.random.default_rng([seed, N, ds, da, H])
    d = pb["X"][:, None, :] - pb["X"][None, :, :]
    Ky_inv = np.stack([np.linalg.inv(np.exp(-0.5 * np.sum(d * d / pb["lambdas"][a], axis=2)) + 1e-2 * np.eye(N)) for a in range(ds)])
    A = rng.standard_normal((ds, ds))
    pb.update(Ky_inv=Ky_inv, U=0.3 * pb["U"], process_var=rng.uniform(0.3, 3.0, ds), init_cov=A @ A.T / ds + 0.3 * np.eye(ds),
              action_var=rng.uniform(0.01, 0.1, da), rng=rng,
              nominal=(np.concatenate([np.eye(ds), np.zeros((ds, da))], axis=1) + 0.05 * rng.standard_normal((ds, ds + da)),
                       0.1 * rng.standard_normal(ds)) if nominal else None)
    return pb


def _pack(G, pb):
    pack = G.GPPack(pb["X"], pb["Y"], pb["Ky_inv"], pb["lambdas"], pb["sigma_f"], nominal=pb["nominal"])
    pack.set_noise(init_cov=pb["init_cov"], action_var=pb["action_var"] if pb["da"] else None, process_var=pb["process_var"])
    return pack


def _rollout(pack, x0, U, cp, grad=True, full=False):
    """gpmpc_rollout / gpmpc_rollout_fullcov through the C ABI (an empty U still hands over a pointer), outputs pre-filled with NaN."""
    from gaussian_process_mpc_amd import _lib
    B, H, da = U.shape
    ds = pack.ds
    flags = _lib.WANT_GRAD if grad else 0
    x0d, Ud = _dev(x0), _dev(U)
    means, cost, g = _nan(B, H + 1, ds), _nan(B), _nan(B, H, da) if grad else None
    L = _L()
    if full:
        if not pack.fullcov:
            pack.enable_fullcov()
        second = _nan(B, H + 1, ds, ds)
        ws = pack.workspace(L.gpmpc_rollout_fullcov_workspace_bytes(pack.handle, B, H, flags))
        _check(L.gpmpc_rollout_fullcov(pack.handle, B, H, _vp(x0d), _vp(Ud), ctypes.byref(cp.c), flags, _vp(means), _vp(second), _vp(cost), _vp(g),
                                       ctypes.c_void_p(ws.data_ptr()), ws.numel(), _sp()), "gpmpc_rollout_fullcov")
    else:
        second = _nan(B, H + 1, ds)
        ws = pack.workspace(L.gpmpc_rollout_workspace_bytes(pack.handle, B, H, flags))
        _check(L.gpmpc_rollout(pack.handle, B, H, _vp(x0d), _vp(Ud), ctypes.byref(cp.c), flags, _vp(means), _vp(second), _vp(cost), _vp(g),
                               ctypes.c_void_p(ws.data_ptr()), ws.numel(), _sp()), "gpmpc_rollout")
    torch.cuda.synchronize()
    out = {"cost": _np(cost, B), "means": _np(means, B, H + 1, ds), "covs" if full else "vars": _np(second, *((B, H + 1, ds, ds) if full else (B, H + 1, ds)))}
    if grad:
        out["grad"] = _np(g, B, H, da)
    return out


def _rollout_jac(pack, x0, U):
    B, H, da = U.shape
    ds = pack.ds
    x0d, Ud = _dev(x0), _dev(U)
    means, vars_, jac = _nan(B, H + 1, ds), _nan(B, H + 1, ds), _nan(B, H, 2 * ds, 2 * ds + da)
    ws = pack.workspace(_L().gpmpc_rollout_jac_workspace_bytes(pack.handle, B, H))
    _check(_L().gpmpc_rollout_jac(pack.handle, B, H, _vp(x0d), _vp(Ud), _vp(means), _vp(vars_), _vp(jac), ctypes.c_void_p(ws.data_ptr()),
                                  ws.numel(), _sp()), "gpmpc_rollout_jac")
    torch.cuda.synchronize()
    return _np(means, B, H + 1, ds), _np(vars_, B, H + 1, ds), _np(jac, B, H, 2 * ds, 2 * ds + da)


def _cost_of_case(G, pb, pack, full, sched, q_f, want_cascade=False):
    """Cost parameters of a tail case: non-symmetric R and R_delta, last_u != 0, and a coupled Q (and Q_f) of the tables' generator with
    gamma = -0.9 / max rho(Q Sigma_t) over the steps of a first, risk-neutral rollout's own variances (covariances).  In a rollout only the
    steps next to the largest rho sit at the edge, so most draws of Q never exchange a row there: the draw is the first of 300 whose float64
    emulation ON THOSE VARIANCES exchanges one (want_cascade: more than one in a column, where a draw does) with no comparison closer than
    1.001 -- an input chosen from the reference side; the caller asserts the exchange again on what the rollout under test returned."""
    ds, da, H, B, rng = pb["ds"], pb["da"], pb["H"], pb["B"], pb["rng"]
    c = dict(ds=ds, da=da, H=H, B=B, Q=np.eye(ds), Q_f=None, R=C.gen_R(rng, da), Rd=C.gen_R(rng, da),
             last_u=rng.standard_normal(da), x_ref=0.5 * rng.standard_normal(ds), u_ref=0.5 * rng.standard_normal(da), X_ref=None, U_ref=None, gamma=0.0)
    if sched:
        c["X_ref"], c["U_ref"] = 0.5 * rng.standard_normal((H + 1, ds)), 0.5 * rng.standard_normal((H, da))
    first = _rollout(pack, pb["x0"], pb["U"], _cost_params(G, c), grad=False, full=full)
    S = first["covs"] if full else np.stack([np.diag(v) for v in first["vars"].reshape(-1, ds)]).reshape(B, H + 1, ds, ds)
    fallback = None
    for seed in range(300):
        qr = np.random.default_rng([seed, ds, 4242])
        Q, Q_f = C.gen_Q(qr, ds), C.gen_Q(qr, ds) if q_f else None
        _, Qs = C.schedule_rows(H, ds, None, None, Q, Q_f)
        rho = C.spectral_radius(np.broadcast_to(Qs, (B, H + 1, ds, ds)).reshape(-1, ds, ds), S.reshape(-1, ds, ds))
        gamma = -0.9 / float(rho.max())
        em = C.emulate_terms("fc" if full else "diag", first["means"], S if full else first["vars"], gamma, Q, c["x_ref"], c["X_ref"], Q_f)
        if ds > 1 and not (em["swaps"].any() and em["margin"].min() >= 1.001):
            continue
        if fallback is None:
            fallback = (Q, Q_f, gamma)
        if ds < 3 or not want_cascade or (em["swaps"] > 1).any():
            break
    else:
        assert fallback is not None, "no draw of Q exchanges a row on these variances"
        Q, Q_f, gamma = fallback
    c.update(Q=Q, Q_f=Q_f, gamma=gamma)
    return c


def _lds_all_fits(ds, da, H):
    """The size rule of the tail's launcher: the Jacobians of all steps beside the cost terms within 48 KiB of LDS."""
    lds0 = 8 * ((H + 1) * (1 + 2 * ds) + H * da + H)
    return lds0 + 8 * 2 * ds * (2 * ds + da) * H <= 48 * 1024


TAIL = [  # (N, ds, da, H, B, nominal, sched, q_f)
    (8, 1, 1, 5, 3, False, False, False), (17, 2, 1, 5, 3, False, False, False), (24, 3, 1, 5, 3, False, True, True),
    (33, 4, 1, 1, 3, False, False, False), (40, 5, 1, 5, 3, True, False, False), (21, 6, 1, 33, 2, False, False, False),
    (30, 7, 1, 5, 3, False, True, False), (36, 8, 0, 4, 3, False, False, False), (25, 3, 5, 4, 3, True, True, True),
    (20, 7, 1, 30, 2, False, False, False), (40, 4, 1, 100, 2, False, True, True)]


@pytest.mark.parametrize("N,ds,da,H,B,nominal,sched,q_f", TAIL, ids=["N%d-ds%d-da%d-H%d%s%s" % (t[0], t[1], t[2], t[3], "-nom" if t[5] else "",
                                                                                                "-sched" + ("Qf" if t[7] else "") if t[6] else "") for t in TAIL])
def test_fused_tail_cost_and_gradient(G, N, ds, da, H, B, nominal, sched, q_f):
    """k_roll_tail<ALLJ, DS, NOM, SCHED>: state_cost_diag, input_cost_step and both reverse sweeps (all Jacobians in LDS; streaming, for
    (7, 1, 30) and (4, 1, 100)) on a real rollout whose variances are of order one, so that I + gamma Q diag(var) pivots -- asserted from the
    emulation on the variances the GPU returned.  H = 1 and H = 33: the 32 state-cost workers idle, or take a second round."""
    pb = _problem(3, N, ds, da, H, B, nominal)
    pack = _pack(G, pb)
    c = _cost_of_case(G, pb, pack, False, sched, q_f)
    cs = _schedule(G, c) if sched else None
    cp = _cost_params(G, c, cs)
    r = _rollout(pack, pb["x0"], pb["U"], cp)
    r0 = _rollout(pack, pb["x0"], pb["U"], cp, grad=False)
    assert _same(r0["cost"], r["cost"]) and _same(r0["means"], r["means"]) and _same(r0["vars"], r["vars"])
    streaming = not _lds_all_fits(ds, da, H)
    assert streaming == ((ds, da, H) in ((7, 1, 30), (4, 1, 100)))
    covs = np.stack([np.diag(v) for v in r["vars"].reshape(-1, ds)]).reshape(B, H + 1, ds, ds)
    kw = dict(C.call_kwargs(c))
    ref = C.cost_terms(r["means"], covs, pb["U"], **kw)
    assert np.all(ref["det"] > 0)
    em = C.emulate_terms("diag", r["means"], r["vars"], c["gamma"], c["Q"], c["x_ref"], c["X_ref"], c["Q_f"])
    assert em["margin"].min() >= C.TIE
    swapped, odd, even, _ = C.swap_summary(em["swaps"])
    print("  ds %d: columns swapped %s, kappa up to %.1f, gamma %.3g" % (ds, sorted(swapped), float(ref["kappa"].max()), c["gamma"]))
    assert ds == 1 or swapped, "no row exchange on the variances the rollout returned"
    f = C.input_terms(pb["U"], c["R"], c["Rd"], c["last_u"], c["u_ref"] if c["U_ref"] is None else c["U_ref"], dtype=np.float64)
    pool = _Pool()
    pool.add("state_cost_diag", "value", C.k_of(r["cost"], ref["value"], ref["A_value"]),
             C.k_of(em["value_state"].sum(1) + f["value"], ref["value"], ref["A_value"]))
    if da:
        mj, vj, J = _rollout_jac(pack, pb["x0"], pb["U"])
        assert _same(mj, r["means"]) and _same(vj, r["vars"]), "gpmpc_rollout_jac does not return the rollout's own means and variances"
        gU, _ = C.sweep(J, ref["dmu"], ref["dvar"])
        aU, _ = C.sweep_unit(J, ref["A_dmu"], ref["A_dvar"])
        fU, _ = C.sweep(J, em["dmu"], em["dvar"], dtype=np.float64)
        form = "tail sweep, streaming" if streaming else "tail sweep, all in LDS"
        pool.add(form, "grad", C.k_of(r["grad"], gU + ref["dU"], aU + ref["A_dU"]), C.k_of(fU + f["dU"], gU + ref["dU"], aU + ref["A_dU"]))
    pool.judge("fused tail")
    if cs is not None:
        cs.close()


_FC = {}


def _fc_case(G, ds, sched):
    """One full-covariance rollout (cached for the module): the rollout, its long double terms and the emulation of fc_state_cost."""
    if (ds, sched) not in _FC:
        pb = _problem(5 + sched, 12 + 4 * ds, ds, 1, 5, 3)
        pack = _pack(G, pb)
        c = _cost_of_case(G, pb, pack, True, sched, sched, want_cascade=True)
        cs = _schedule(G, c) if sched else None
        cp = _cost_params(G, c, cs)
        r = _rollout(pack, pb["x0"], pb["U"], cp, full=True)
        r0 = _rollout(pack, pb["x0"], pb["U"], cp, grad=False, full=True)
        if cs is not None:
            cs.close()
        ref = C.cost_terms(r["means"], r["covs"], pb["U"], **C.call_kwargs(c))
        em = C.emulate_terms("fc", r["means"], r["covs"], c["gamma"], c["Q"], c["x_ref"], c["X_ref"], c["Q_f"])
        _FC[ds, sched] = (pb, c, r, r0, ref, em)
    return _FC[ds, sched]


@pytest.mark.parametrize("ds", range(1, 7))
def test_fullcov_tail_cost(G, ds):
    """k_fc_tail<ds, SCHED>: fc_state_cost and fc_input_cost on rollout_fullcov's own means and covariances under the same noise model (a
    non-diagonal init_cov), plain and with a schedule and Q_f; swaps asserted on the returned covariances."""
    pool = _Pool()
    for sched in (False, True):
        pb, c, r, r0, ref, em = _fc_case(G, ds, sched)
        assert _same(r0["cost"], r["cost"])
        assert np.all(ref["det"] > 0)
        assert em["margin"].min() >= C.TIE
        swapped, _, _, cascade = C.swap_summary(em["swaps"])
        print("  ds %d%s: columns swapped %s, cascade %s, kappa up to %.1f" % (ds, " sched" if sched else "", sorted(swapped), cascade, float(ref["kappa"].max())))
        assert ds == 1 or swapped, "no row exchange on the covariances the rollout returned"
        f = C.input_terms(pb["U"], c["R"], c["Rd"], c["last_u"], c["u_ref"] if c["U_ref"] is None else c["U_ref"], dtype=np.float64)
        pool.add("fc_state_cost", "value", C.k_of(r["cost"], ref["value"], ref["A_value"]),
                 C.k_of(em["value_state"].sum(1) + f["value"], ref["value"], ref["A_value"]))
        assert np.all(np.isfinite(r["grad"]))
    pool.judge("full-covariance tail ds %d" % ds)


@pytest.mark.parametrize("ds", range(1, 7))
def test_fullcov_tail_gradient_against_the_complex_step(G, ds):
    """The gradient of k_fc_tail (fc_state_cost's d/dmu and symmetrised d/dSigma through the four-lanes-per-entry sweep, fc_input_cost's
    d/dU with R_delta, both neighbours and last_u != 0) on a pivoting cost: against the long double complex step of the CPU port on the
    constants the kernels read (pack.beta(), pack.weights()) under the same noise model, with the floor convention of
    tests/test_gpu_accuracy.py -- the same statistic for the double complex build of that port.  The port knows x_ref, u_ref, a general Q
    and R; the R_delta term does not depend on the state, so its value and gradient are added to both builds from the long double
    input_terms.  The port knows no schedule: the SCHED instance is held to the plain one, whose bits a schedule of constant rows must return
    on the pivoting cost too."""
    from oracle import cport
    pb = _problem(9, 12 + 4 * ds, ds, 1, 4, 2)
    pack = _pack(G, pb)
    c = _cost_of_case(G, pb, pack, True, False, False)
    H = pb["H"]
    r = _rollout(pack, pb["x0"], pb["U"], _cost_params(G, c), full=True)
    cs = _schedule(G, dict(c, X_ref=np.tile(c["x_ref"], (H + 1, 1)), U_ref=np.tile(c["u_ref"], (H, 1)), Q_f=None))
    rs = _rollout(pack, pb["x0"], pb["U"], _cost_params(G, c, cs), full=True)
    cs.close()
    assert all(_same(rs[q], r[q]) for q in r), "k_fc_tail: a constant schedule does not return the bits of no schedule"
    em = C.emulate_terms("fc", r["means"], r["covs"], c["gamma"], c["Q"], c["x_ref"])
    assert em["margin"].min() >= C.TIE and (ds == 1 or em["swaps"].any())
    consts = pack.beta().cpu().numpy(), pack.weights().cpu().numpy()
    pbc = dict(pb, Q=c["Q"], R=c["R"], x_ref=c["x_ref"], u_ref=c["u_ref"])
    kw = dict(full=True, nthreads=4, init_cov=pb["init_cov"], action_var=pb["action_var"], process_var=pb["process_var"])
    cld = cport.given_rollout(pbc, *consts, c["gamma"], prec="cld", **kw)
    cd = cport.given_rollout(pbc, *consts, c["gamma"], prec="cd", **kw)
    assert np.all(np.isfinite(cld["cost"])) and np.all(np.isfinite(cld["grad"]))
    with_d, without = C.input_terms(pb["U"], c["R"], c["Rd"], c["last_u"], c["u_ref"]), C.input_terms(pb["U"], c["R"], None, None, c["u_ref"])
    dv, dg = with_d["value"] - without["value"], with_d["dU"] - without["dU"]              # the R_delta term, long double
    assert np.abs(dg).min() > 0
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, dtype=C.LD) - b) / np.linalg.norm(b))  # noqa: E731
    k = {"cost": max(rel(r["cost"][b], cld["cost"][b] + dv[b]) for b in range(2)),
         "cost_floor": max(rel(cd["cost"][b] + dv[b], cld["cost"][b] + dv[b]) for b in range(2)),
         "grad": max(rel(r["grad"][b], cld["grad"][b] + dg[b]) for b in range(2)),
         "grad_floor": max(rel(cd["grad"][b] + dg[b], cld["grad"][b] + dg[b]) for b in range(2))}
    print("  ds %d: cost %.3g (floor %.3g), gradient in norm %.3g (floor %.3g), columns swapped %s" %
          (ds, k["cost"], k["cost_floor"], k["grad"], k["grad_floor"], sorted(C.swap_summary(em["swaps"])[0])))
    for q in ("cost", "grad"):
        w = _WORST.get(("k_fc_tail complex step", q), (0.0, 0.0))
        _WORST["k_fc_tail complex step", q] = max(w, (k[q], k[q + "_floor"]))
        # (a double cannot stand closer than 2^-53 to the long double value: a floor of exactly 0 over two trajectories is two roundings
        #  that coincided, not a sharper yardstick)
        assert k[q] <= 10 * max(k[q + "_floor"], C.U53), (q, k)
        assert k[q] <= C.CAP_REL["fc " + q], (q, k)


def test_the_cascade_ran(G):
    """At least one full-covariance case took more than one exchange in one column: fc_state_cost's own rule, which the other three
    eliminations do not have."""
    assert any(C.swap_summary(_fc_case(G, ds, sched)[5]["swaps"])[3] for ds in range(3, 7) for sched in (False, True))
