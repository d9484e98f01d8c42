"""The yardstick of the cost path (tests/cost_reference.py) pinned on the CPU, the float64 floor K_ref of the four eliminations as the kernels
write them, the conditions the input tables must meet for the GPU assertions of tests/test_gpu_cost.py to mean something, and what the new
tables see that the inputs of the existing tests do not.

K = |x - long double| / (2^-53 A) with the units of tests/cost_reference.py.  K_ref measured here (plain float64 numpy, every call of the
host tables, ds = 2 ... 8: kappa from 1 to 121, 16 slots a call), worst per form and output:
    state_cost / state_cost_sched (largest entry, one row swap)      value 1.94   d/dmu 2.97   d/dSigma 3.23
    fc_state_cost (cascade of compare-and-swaps, symmetrised)        value 1.94   d/dmu 2.97   d/dSigma 3.23
    state_cost_diag (diagonal Sigma)                                 value 2.74   d/dmu 2.98   d/dvar 3.52
    input cost                                                       value 2.45   d/dU 1.76
    reverse sweep                                                    gU 1.91      gx0 0.88
The long double form lies within 0.003 unit of the 50-digit form; CPU torch autograd of the reference's expression within 2.5 units.

The defect table (emulated in the float64 forms, one at a time; "old" = the matrices of test_cost_torch_gradients_general_covariance, the
fixture g5_cost.npz and diagonal variances of 1e-3 ... 6e-2, judged by the bands of their tests; "new" = K > 10 K_ref on a call of the tables):
    defect                                  old inputs                                              new tables
    no sign flip of det on a swap           g5 only (state_cost, ds = 2, column 0): NaN             every form, every ds >= 2
    swap on the left ds columns only        none (g5 swaps, but returns the same bits: see below)   every form, every ds >= 2
    pivot chosen without fabs               none                                                    'tiny' calls only, every form, ds >= 2 (*)
    Z for Z^T in d/dSigma                   seen (non-symmetric Sigma, ds = 3): no gap              full / sched, every ds >= 2
    -(qn + qtn) neighbour term dropped      seen (R_delta on, u.grad checked): no gap               seen
    last_u ignored at j = 0                 seen (last_traj != 0): no gap                           seen
    Q_f at step H - 1                       no schedule in these inputs (test_gpu_tracking's part)  seen
    seed of step t - 1 dropped in the sweep not evaluated here (autograd round trips on fixtures)   seen
Z for Z^T does not exist as a defect of state_cost_diag (a diagonal) or fc_state_cost (symmetrised): asserted below.
(*) a pivot chosen without fabs is still a valid elimination, only a less stable one: on the gamma = -0.9 / rho calls (negative entries below
a positive diagonal) it never exchanges a row and stays within 1.7 K_ref.  The 'tiny' calls put 1e-6 on the leading diagonal above entries of
order -1: there it loses six digits (more than 100 K_ref), which is what makes it visible to a rounding-error budget and to nothing else.
"""
import numpy as np
import pytest

import cost_reference as C

DS = list(range(2, 9))
_KREF = {}


def _ref(c):
    return C.cost_terms(c["means"], c["covs"], c["U"], **C.call_kwargs(c))


def _em(form, c, defect=None):
    return C.emulate_terms(form, c["means"], c["vars"] if form == "diag" else c["covs"], c["gamma"], c["Q"], c["x_ref"], c["X_ref"], c["Q_f"], defect)


def _finite(em):
    """A NaN (the logarithm of a negative determinant) counts as far away."""
    return {k: np.where(np.isfinite(v), v, 1e300) if v.dtype.kind == "f" else v for k, v in em.items()}


@pytest.fixture(scope="module")
def tables():
    """Per (ds, diag): the calls with their long double reference."""
    out = {}
    for ds in DS:
        for diag in (False, True):
            out[ds, diag] = [(c, _ref(c)) for c in C.host_table(ds, diag)]
    return out


def test_long_double_has_the_precision_the_units_assume():
    assert np.finfo(C.LD).eps < 1.1e-19


@pytest.mark.parametrize("ds", [1] + DS)
def test_long_double_form_agrees_with_50_digits(ds):
    """Householder QR in long double against det / inverse of mpmath at 50 digits: within 0.02 unit on every output, the pivoting slots, the
    gamma > 0 and the gamma = 0 call."""
    import mpmath as mp
    worst = 0.0
    for fam in ("neg", "pos", "zero"):
        c = C.gen_call(1, ds, 1, 3, 1, fam)
        r = _ref(c)
        xr, Qs = C.schedule_rows(3, ds, c["x_ref"], None, c["Q"], None)
        for i in range(4):
            with mp.workdps(50):
                e = [mp.mpf(float(a)) - mp.mpf(float(b)) for a, b in zip(c["means"][0, i], xr[i])]
            m = C.state_mp(c["Q"], c["covs"][0, i], e, c["gamma"])
            with mp.workdps(50):
                def k(ld, mpv, A):
                    return float(abs(mp.mpf(float(ld)) + mp.mpf(float(ld - C.LD(float(ld)))) - mpv) / (mp.mpf(2) ** -53 * mp.mpf(float(A))))
                worst = max(worst, k(r["value_state"][0, i], m["value"], r["A_value_state"][0, i]))
                assert abs(float(r["kappa"][0, i]) / float(m["kappa"]) - 1) < 1e-12 and float(m["det"]) > 0
                for a in range(ds):
                    worst = max(worst, k(r["dmu"][0, i, a], m["dmu"][a], r["A_dmu"][0, i, a]))
                    for b in range(ds):
                        worst = max(worst, k(r["dsig"][0, i, a, b], m["dsig"][a][b], r["A_dsig"][0, i, a, b]))
    print("ds = %d: long double against 50 digits, worst %.2e unit" % (ds, worst))
    assert worst < 0.02


def test_long_double_subtracts_the_reference_without_rounding_the_tables_apart():
    """e = mu - x_ref differs between a float64 and a long double subtraction by one float64 rounding of e: the emulation and the kernels
    round it, the reference does not; the units carry it (|e| enters every unit)."""
    c = C.gen_call(1, 3, 1, 3, 1, "neg")
    e64 = c["means"] - c["x_ref"]
    eld = c["means"].astype(C.LD) - c["x_ref"].astype(C.LD)
    assert np.all(np.abs(e64 - eld) <= 2.0 ** -53 * np.abs(eld))


@pytest.mark.parametrize("ds", [2, 5, 8])
def test_closed_form_derivatives_agree_with_central_differences_at_50_digits(ds):
    """d/dmu and the NON-symmetrised d/dSigma_kl of the reference's own expression (inverse of Q, inverse of Q^-1 + gamma Sigma) by central
    differences with h = 1e-20 at 50 digits, on the slot of a pivoting call closest to the edge."""
    import mpmath as mp
    c = C.gen_call(2, ds, 1, 3, 1, "neg")
    r = _ref(c)
    i = int(np.argmax(r["kappa"][0]))
    with mp.workdps(50):
        Q, S = mp.matrix(c["Q"].tolist()), mp.matrix(c["covs"][0, i].tolist())
        mu, xr, g = mp.matrix(c["means"][0, i].tolist()), mp.matrix(c["x_ref"].tolist()), mp.mpf(float(c["gamma"]))
        m = C.state_mp(c["Q"], c["covs"][0, i], [mu[k] - xr[k] for k in range(ds)], c["gamma"])
        assert abs(C.state_value_mp(Q, S, mu, xr, g) - m["value"]) < mp.mpf(10) ** -40 * abs(m["value"])
        h = mp.mpf(10) ** -20
        scale = max(abs(v) for row in m["dsig"] for v in row)
        for k in range(ds):
            d = mp.zeros(ds, 1)
            d[k] = h
            fd = (C.state_value_mp(Q, S, mu + d, xr, g) - C.state_value_mp(Q, S, mu - d, xr, g)) / (2 * h)
            assert abs(fd - m["dmu"][k]) < mp.mpf(10) ** -25 * max(abs(v) for v in m["dmu"])
            for l in range(ds):
                D = mp.zeros(ds, ds)
                D[k, l] = h
                fd = (C.state_value_mp(Q, S + D, mu, xr, g) - C.state_value_mp(Q, S - D, mu, xr, g)) / (2 * h)
                assert abs(fd - m["dsig"][k][l]) < mp.mpf(10) ** -25 * scale


@pytest.mark.parametrize("ds,da", [(1, 1), (3, 2), (6, 3), (8, 0)])
def test_agrees_with_torch_autograd_of_the_reference_expression(ds, da):
    """Value, d/dmu, non-symmetrised d/dSigma and d/dU against CPU torch autograd of the expression of src/mpc.py:179-198 (schedule rows and
    Q_f included), in K: torch's fp64 (an inverse of Q, an inverse of Q^-1 + gamma Sigma, a determinant by LU) measures 0.1 ... 2.5 units and
    is held to 10."""
    import torch
    for fam, sched in (("neg", True), ("pos", False)):
        c = C.gen_call(3, ds, da, 4, 2, fam, sched=sched, q_f=sched)
        r = _ref(c)
        H, B = c["H"], c["B"]
        xr, Qs = C.schedule_rows(H, ds, c["x_ref"], c["X_ref"], c["Q"], c["Q_f"])
        ur = np.broadcast_to(c["u_ref"], (H, da)) if c["U_ref"] is None else c["U_ref"]
        x = torch.tensor(c["means"], requires_grad=True)
        s = torch.tensor(c["covs"], requires_grad=True)
        u = torch.tensor(c["U"], requires_grad=True)
        I, g = torch.eye(ds, dtype=torch.float64), c["gamma"]
        tot = []
        for b in range(B):
            v = 0.0
            for i in range(H + 1):
                Qt = torch.tensor(Qs[i])
                e = x[b, i] - torch.tensor(xr[i])
                v = v + (1 / g) * torch.log(torch.det(I + g * Qt @ s[b, i])) + e @ torch.linalg.inv(torch.linalg.inv(Qt) + g * s[b, i]) @ e
            if da:
                Rt, Rdt = torch.tensor(c["R"]), torch.tensor(c["Rd"])
                for j in range(H):
                    d = u[b, j] - torch.tensor(ur[j])
                    v = v + d @ Rt @ d
                du = torch.diff(torch.cat((torch.tensor(c["last_u"])[None, :], u[b]), dim=0), dim=0)
                for j in range(H):
                    v = v + du[j] @ Rdt @ du[j]
            tot.append(v)
        torch.stack(tot).sum().backward()
        k = {"value": C.k_of(torch.stack(tot).detach().numpy(), r["value"], r["A_value"]), "dmu": C.k_of(x.grad.numpy(), r["dmu"], r["A_dmu"]),
             "dsig": C.k_of(s.grad.numpy(), r["dsig"], r["A_dsig"]), "dU": C.k_of(u.grad.numpy() if da else np.zeros((B, H, 0)), r["dU"], r["A_dU"])}
        print("ds %d da %d %s: torch autograd K %s" % (ds, da, fam, {a: round(b, 2) for a, b in k.items()}))
        assert max(k.values()) < 10, k


def test_gamma_zero_is_the_limit():
    """tr(Q Sigma) + e^T Q e and Z = Q: the limit of the 50-digit form (gamma = 1e-12 is within 1e-9 of it)."""
    import mpmath as mp
    c = C.gen_call(0, 4, 1, 2, 1, "zero")
    r = _ref(c)
    e = (c["means"][0, 1] - c["x_ref"]).tolist()
    m = C.state_mp(c["Q"], c["covs"][0, 1], e, 1e-12)
    z = C.state_mp(c["Q"], c["covs"][0, 1], e, 0.0)
    with mp.workdps(50):
        assert abs(m["value"] - z["value"]) < 1e-9 * abs(z["value"])
        assert all(abs(m["dsig"][k][l] - z["dsig"][k][l]) < 1e-9 for k in range(4) for l in range(4))
    rl = C.state_terms(c["Q"], c["covs"][0, 1:2], (c["means"][0, 1:2] - c["x_ref"]), 0.0)
    assert abs(float(rl["value"][0]) - float(z["value"])) < 1e-15 * float(rl["A_value"][0])
    assert np.array_equal(rl["dsig"][0], c["Q"].T.astype(C.LD)) and float(r["kappa"].max()) == 1.0


@pytest.mark.parametrize("diag", [False, True], ids=["full_sigma", "diag_sigma"])
@pytest.mark.parametrize("ds", DS)
def test_input_conditions_and_k_ref(tables, ds, diag):
    """ASSERTED per state dimension and per elimination form, from the float64 emulation: every column 0 ... ds - 2 swaps in some case; some
    slot has an odd number of swaps and (ds >= 3: at ds = 2 only column 0 can swap, once) some slot an even number >= 2; every slot has
    det > 0 in the reference; kappa spans from below 2 to above 30; no pivot comparison is closer than 1 + 1e-6, so the kernels (fused
    multiply-adds, another order) choose the rows the emulation chooses.  The cascade takes more than one swap in one column at every
    ds >= 3 where this table reaches it (asserted over all ds together in test_the_cascade_is_reached).  Records K_ref."""
    for form in (("diag",) if diag else ("full", "sched", "fc")):
        cols, odd, even, kmin, kmax = set(), False, False, np.inf, 0.0
        for c, r in tables[ds, diag]:
            em = _em(form, c)
            a, b, e2, _ = C.swap_summary(em["swaps"])
            cols |= a
            odd |= b
            even |= e2
            assert np.all(r["det"] > 0) and np.all(np.isfinite(r["value"]))
            assert em["margin"].min() >= C.TIE, (form, ds, em["margin"].min())
            assert np.all(np.sign(em["det"]) > 0) if em.get("det") is not None else True
            kmin, kmax = min(kmin, float(r["kappa"].min())), max(kmax, float(r["kappa"].max()))
            for name, v in C.k_state(form, em, r).items():
                _KREF[form, name] = max(_KREF.get((form, name), 0.0), v)
                assert v < 10, (form, name, v)                      # the floor itself (measured 0.8 ... 3.5): an emulation that loses more is wrong
        assert cols == set(range(ds - 1)), (form, ds, sorted(cols))
        assert odd and (even or ds == 2), (form, ds)
        assert kmin < 2 and kmax > 30, (form, ds, kmin, kmax)
    print("\n  K_ref so far: " + ", ".join("%s %s %.2f" % (k[0], k[1], v) for k, v in sorted(_KREF.items())))


def test_the_cascade_is_reached(tables):
    """fc_state_cost exchanges row k with EVERY later row that beats the current one: more than one exchange in one column, and so a
    permutation and a number of sign flips that differ from the other three forms on the same matrix."""
    n = 0
    for ds in DS[1:]:
        for c, r in tables[ds, False]:
            fc, full = _em("fc", c), _em("full", c)
            n += int(np.sum((fc["swaps"] > 1).any(-1)))
            assert np.all(full["swaps"] <= 1)
    assert n >= 5, n


def test_sched_is_the_arithmetic_of_full(tables):
    """state_cost_sched restates state_cost with the swap as predicated moves: in float64 the two emulations are one."""
    c, _ = tables[4, False][0]
    a, b = _em("full", c), _em("sched", c)
    assert all(np.array_equal(a[k], b[k]) for k in ("value_state", "dmu", "dsig"))


def test_input_cost_and_sweep_floor():
    """K_ref of the input cost (general R, R_delta, last_u, schedule rows) and of the reverse sweep in plain float64."""
    worst = {}
    for ds, da, H, B in ((1, 1, 1, 1), (3, 3, 7, 3), (8, 8, 9, 3), (2, 5, 2, 1)):
        c = C.gen_call(5, ds, da, H, B, "neg", sched=True)
        r = C.input_terms(c["U"], c["R"], c["Rd"], c["last_u"], c["U_ref"])
        f = C.input_terms(c["U"], c["R"], c["Rd"], c["last_u"], c["U_ref"], dtype=np.float64)
        worst["input value"] = max(worst.get("input value", 0), C.k_of(f["value"], r["value"], r["A_value"]))
        worst["input dU"] = max(worst.get("input dU", 0), C.k_of(f["dU"], r["dU"], r["A_dU"]))
        v = C.gen_vjp(5, ds, da, H, B)
        for gm, gv in ((v["gm"], v["gv"]), (None, v["gv"]), (v["gm"], None)):
            (gU, gx0), (aU, ax0) = C.sweep(v["J"], gm, gv), C.sweep_unit(v["J"], gm, gv)
            fU, fx0 = C.sweep(v["J"], gm, gv, dtype=np.float64)
            worst["sweep gU"] = max(worst.get("sweep gU", 0), C.k_of(fU, gU, aU))
            worst["sweep gx0"] = max(worst.get("sweep gx0", 0), C.k_of(fx0, gx0, ax0))
    print("\n  K_ref: " + ", ".join("%s %.2f" % kv for kv in sorted(worst.items())))
    assert worst["input value"] < 4 and worst["input dU"] < 4 and worst["sweep gU"] < 6 and worst["sweep gx0"] < 6


# ---------------------------------------------------------------------------------------------------------------------------------------
# what the existing inputs exercise, and what each defect would cost on them
# ---------------------------------------------------------------------------------------------------------------------------------------
def _autograd_test_inputs():
    """The matrices of tests/test_gpu_autograd.py::test_cost_torch_gradients_general_covariance: the same generator, the same draws."""
    rng = np.random.default_rng(5)
    ds, da, H = 3, 2, 4
    A = rng.standard_normal((ds, ds))
    Q = A @ A.T + ds * np.eye(ds)
    R = np.diag(rng.uniform(0.1, 1.0, da))
    Rd = np.diag(rng.uniform(0.1, 1.0, da))
    out = []
    for gamma in (-0.05, 1e-5, 0.7):
        last = rng.standard_normal(H * da)
        x_ref, u_ref = rng.standard_normal(ds), rng.standard_normal(da)
        xs = rng.standard_normal((H + 1, ds))
        ss = 0.05 * rng.standard_normal((H + 1, ds, ds)) + 0.2 * np.eye(ds)
        us = rng.standard_normal((H, da))
        out.append(dict(ds=ds, da=da, H=H, B=1, gamma=gamma, Q=Q, Q_f=None, R=R, Rd=Rd, last_u=last[:da], x_ref=x_ref, u_ref=u_ref,
                        X_ref=None, U_ref=None, means=xs[None], covs=ss[None], U=us[None]))
    return out


def _g5_inputs(golden):
    z = golden("g5_cost.npz")
    a = dict(gamma=1.0, Q=z["a_Q"], x_ref=z["a_xref"], means=z["a_x"][None], covs=z["a_sig"][None], X_ref=None, Q_f=None)
    b = dict(gamma=1.1, Q=z["a_Q"], x_ref=z["a_xref"], means=z["b_x"][None], covs=z["b_sig"][None], X_ref=None, Q_f=None)
    return [a, b]


def _small_variance_inputs(ds):
    """Diagonal variances of 1e-3 ... 6e-2, the range of every rollout test, under a COUPLED weight of the tables (the rollout tests
    themselves use Q = 0.1 I or the fixtures' weights) and the risk parameters those tests use."""
    rng = np.random.default_rng(100 + ds)
    out = []
    for gamma in (-1.0, 1e-5, 1.0):
        v = rng.uniform(1e-3, 6e-2, (3, 8, ds))
        out.append(dict(gamma=gamma, Q=C.gen_Q(rng, ds), x_ref=np.zeros(ds), means=rng.standard_normal((3, 8, ds)), vars=v,
                        covs=np.stack([np.diag(r) for r in v.reshape(-1, ds)]).reshape(3, 8, ds, ds), X_ref=None, Q_f=None))
    return out


def test_the_existing_inputs_never_pivot_the_templated_eliminations(golden):
    """The statement the new tables rest on: the matrices of test_cost_torch_gradients_general_covariance produce no swap (condition numbers
    at most 1.83), g5_cost.npz produces only the ds = 2, column-0 swap (through the run-time state_cost, value only), and variances of
    1e-3 ... 6e-2 produce none in any form."""
    kap = 0.0
    for c in _autograd_test_inputs():
        assert not _em("full", c)["swaps"].any()
        for i in range(c["H"] + 1):
            kap = max(kap, np.linalg.cond(np.eye(3) + c["gamma"] * c["Q"] @ c["covs"][0, i]))
    assert kap < 1.84
    cols = set()
    for c in _g5_inputs(golden):
        sw = _em("full", c)["swaps"]
        assert sw.shape[-1] == 2
        cols |= C.swap_summary(sw)[0]
    assert cols == {0}
    for ds in DS:
        for c in _small_variance_inputs(ds):
            for form in ("sched", "diag", "fc"):
                assert not _em(form, c)["swaps"].any()


@pytest.mark.parametrize("defect", C.DEFECTS_ELIM)
def test_elimination_defects_old_inputs_and_new_tables(tables, golden, defect):
    """Each defect of the elimination, emulated in the float64 forms.  Old inputs: bit-identical outputs wherever nothing swaps (nothing
    to see), except where stated; new tables: K > 10 K_ref of the same call for every form the defect exists in, at every ds >= 2."""
    forms = ("full", "sched") if defect == "z_for_zt" else C.FORMS
    # -- old inputs
    if defect == "z_for_zt":
        seen = False
        for c in _autograd_test_inputs():
            ok, bad = _em("full", c), _em("full", c, defect)
            seen |= not np.allclose(bad["dsig"], ok["dsig"], rtol=1e-7, atol=1e-9)        # the band of the existing test
        assert seen                                                                      # already caught: no gap claimed
        for c, _ in tables[4, False][:2]:                                                # not a defect of the symmetrised / diagonal forms
            np.testing.assert_allclose(_em("fc", c)["dsig"], _em("fc", c, defect)["dsig"], rtol=1e-13, atol=1e-13)
            assert np.array_equal(_em("diag", tables[4, True][0][0])["dvar"], _em("diag", tables[4, True][0][0], defect)["dvar"])
    else:
        for c in _autograd_test_inputs():
            ok, bad = _em("full", c), _em("full", c, defect)
            assert all(np.array_equal(ok[k], bad[k]) for k in ("value_state", "dmu", "dsig"))
        g5 = False
        for c in _g5_inputs(golden):
            ok, bad = _em("full", c), _em("full", c, defect)
            g5 |= not abs(bad["value_state"].sum() - ok["value_state"].sum()) < 1e-9
        # the run-time state_cost IS held by g5 at ds = 2, column 0, value only: that sees the sign of det (NaN) and nothing else -- its
        # errors have equal components and Q e is invariant under the row exchange, so a swap that misses Q returns the same bits
        assert g5 == (defect == "no_sign")
        for ds in DS:
            for c in _small_variance_inputs(ds):
                for form in ("sched", "diag", "fc"):
                    ok, bad = _em(form, c), _em(form, c, defect)
                    assert all(np.array_equal(ok[k], bad[k]) for k in ok if k not in ("swaps", "margin"))
    # -- new tables
    for ds in DS:
        for form in forms:
            caught = 0
            for c, r in tables[ds, form == "diag"]:
                if c["family"] not in ("neg", "tiny"):
                    continue
                kr, kd = C.k_state(form, _em(form, c), r), None
                kd = C.k_state(form, _finite(_em(form, c, defect)), r)
                caught += any(kd[k] > 10 * kr[k] for k in kr)
            assert caught >= 1, (defect, form, ds)


def test_input_cost_schedule_and_sweep_defects():
    """The four defects outside the elimination.  The neighbour term and last_u are ALREADY caught by the inputs of
    test_cost_torch_gradients_general_covariance (R_delta on, last_traj != 0, u.grad within 1e-9): asserted, no gap claimed.  The new tables
    see each of them, Q_f one step early and a dropped seed, far outside 10 K_ref."""
    for c in _autograd_test_inputs():
        ok = C.input_terms(c["U"], c["R"], c["Rd"], c["last_u"], c["u_ref"], dtype=np.float64)
        for d in ("no_neighbour", "no_last_u"):
            bad = C.input_terms(c["U"], c["R"], c["Rd"], c["last_u"], c["u_ref"], dtype=np.float64, defect=d)
            assert not np.allclose(bad["dU"], ok["dU"], rtol=1e-9, atol=1e-11)
    for ds, da, H, B in ((2, 1, 2, 1), (5, 3, 7, 3)):
        c = C.gen_call(6, ds, da, H, B, "neg", sched=True, q_f=True)
        r = _ref(c)
        f = C.input_terms(c["U"], c["R"], c["Rd"], c["last_u"], c["U_ref"], dtype=np.float64)
        kr = max(C.k_of(f["dU"], r["dU"], r["A_dU"]), 0.05)
        for d in ("no_neighbour", "no_last_u"):
            bad = C.input_terms(c["U"], c["R"], c["Rd"], c["last_u"], c["U_ref"], dtype=np.float64, defect=d)
            assert C.k_of(bad["dU"], r["dU"], r["A_dU"]) > 1e6 * kr
        for form in ("sched", "fc"):
            kr = C.k_state(form, _em(form, c), r)
            kd = C.k_state(form, _finite(_em(form, c, "qf_early")), r)
            assert kd["value"] > 1e6 * kr["value"] and kd["dmu"] > 1e6 * kr["dmu"]
        v = C.gen_vjp(6, ds, da, H, B)
        (gU, gx0), (aU, ax0) = C.sweep(v["J"], v["gm"], v["gv"]), C.sweep_unit(v["J"], v["gm"], v["gv"])
        bU, bx0 = C.sweep(v["J"], v["gm"], v["gv"], dtype=np.float64, defect="drop_seed")
        assert C.k_of(bx0, gx0, ax0) > 1e6
        assert H == 1 or C.k_of(bU, gU, aU) > 1e6
