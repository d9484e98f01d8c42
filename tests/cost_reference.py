"""The yardstick of the COST PATH: the risk-sensitive cost (reference src/mpc.py:179-198), its local derivatives, the input cost, a cost
schedule and the reverse sweep over given step Jacobians, restated plainly in extended precision, next to float64 emulations of the four
hand-written eliminations of the library as they are written (their pivot rules included).

    state term      (1/g) log det(I + g Q S) + e^T Z e,   Mx = I + g Q S,   Z = Mx^-1 Q = (Q^-1 + g S)^-1,   e = mu - x_ref
    d/dmu           (Z + Z^T) e
    d/dS_kl         Z_lk - g (Z^T e)_k (Z e)_l                (non-symmetrised: k_cost_full, k_cost_sched)
    symmetrised     1/2 (d/dS + d/dS^T)                        (fc_state_cost)
    d/dvar_k        the diagonal of d/dS                       (state_cost_diag)
    g = 0           tr(Q S) + e^T Q e,  Z = Q

Two forms, neither of them a Gauss-Jordan elimination: `state_mp` takes det, Mx^-1 and Z from mpmath at 50 digits, one matrix at a time;
`state_terms` is the batched numpy.longdouble form (Householder QR, det = (-1)^reflections prod diag R, Z by back substitution) that
tests/test_host_cost.py pins to the first.

Beside every value stands its error unit A, a function of the REFERENCE alone, and K = |x - reference| / (2^-53 A).  With
W = |Mx^-1| (I + |g| |Q| |S|) |Mx^-1| |Q| -- what an elimination of [Mx | Q] can lose in each entry of Z: the absolute terms that form Mx,
carried through the inverse twice; W >= |Z| entry by entry, and W = |Q| at g = 0 -- and kappa = ||Mx||_inf ||Mx^-1||_inf:
    value       kappa ds / |g| + |e|^T W |e|                  (g = 0: sum |Q_kl S_lk| + |e|^T |Q| |e|)     + sum |input terms|
    d/dmu_k     ((W + W^T) |e|)_k
    d/dS_kl     W_lk + |g| ((W^T |e|)_k |Z e|_l + |Z^T e|_k (W |e|)_l)
    d/dU        (|R| + |R|^T) |u - u_ref| and the same with R_delta on both neighbours
    sweep       the same sweep over |J| and the |seeds| (for the fused tails: over the UNITS of the seeds, which bound them)
The first choice, kappa |Z_lk| for an entry of Z, is off by construction: an entry of Z that cancels to 1 % of |Mx^-1| |Q| carries the error of
the terms it cancelled from, and the float64 eliminations sat at K_ref = 30 ... 200 on d/dSigma at ds >= 6 (3 with W, at every ds).
"""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
FORMS = ("full", "sched", "diag", "fc")
DEFECTS_ELIM = ("no_sign", "swap_left", "no_fabs", "z_for_zt")
TIE = 1.0 + 1e-6
NEG_CALLS = 12


# ---------------------------------------------------------------------------------------------------------------------------------------
# extended precision
# ---------------------------------------------------------------------------------------------------------------------------------------
def _qr_inverse(M, rhs):
    """Batched Householder QR of M [n][d][d] in M's dtype: det [n] and M^-1 rhs [n][d][m]."""
    M, rhs = M.copy(), rhs.copy()
    n, d, _ = M.shape
    sign = np.ones(n, dtype=M.dtype)
    for k in range(d):
        x = M[:, k:, k]
        nx = np.sqrt((x * x).sum(1))
        v = x.copy()
        v[:, 0] -= np.where(x[:, 0] >= 0, -nx, nx)
        nv = np.sqrt((v * v).sum(1))
        ok = nv > 0
        v = v / np.where(ok, nv, 1)[:, None]
        M[:, k:, :] -= 2 * v[:, :, None] * np.einsum("ni,nij->nj", v, M[:, k:, :])[:, None, :]
        rhs[:, k:, :] -= 2 * v[:, :, None] * np.einsum("ni,nij->nj", v, rhs[:, k:, :])[:, None, :]
        sign = np.where(ok, -sign, sign)
    det = sign * np.prod(np.einsum("nii->ni", M), axis=1)
    X = np.zeros_like(rhs)
    for i in range(d - 1, -1, -1):
        X[:, i, :] = (rhs[:, i, :] - np.einsum("nj,njm->nm", M[:, i, i + 1:], X[:, i + 1:, :])) / M[:, i, i][:, None]
    return det, X


def state_terms(Q, S, e, gamma, dtype=LD):
    """Q, S [n][ds][ds] (or Q [ds][ds] for all), e [n][ds]: dict of value, dmu, dsig, dsig_sym, dvar, their units A_*, kappa, det; every
    entry [n]...  det <= 0 gives a NaN value, as the reference does."""
    S = np.asarray(S, dtype=dtype)
    n, ds, _ = S.shape
    Q = np.broadcast_to(np.asarray(Q, dtype=dtype), (n, ds, ds))
    e = np.asarray(e, dtype=dtype)
    g = dtype(gamma)
    eye = np.broadcast_to(np.eye(ds, dtype=dtype), (n, ds, ds))
    ae = np.abs(e)
    if gamma == 0:
        Z, kappa, det = Q, np.ones(n, dtype=dtype), np.ones(n, dtype=dtype)
        logterm = np.einsum("nkl,nlk->n", Q, S)
        a_log = np.einsum("nkl,nlk->n", np.abs(Q), np.abs(S))
    else:
        Mx = eye + g * np.einsum("nkl,nlm->nkm", Q, S)
        det, X = _qr_inverse(Mx, np.concatenate([eye, Q], axis=2))
        Mi, Z = X[:, :, :ds], X[:, :, ds:]
        kappa = np.abs(Mx).sum(2).max(1) * np.abs(Mi).sum(2).max(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            logterm = np.log(det) / g
        a_log = kappa * ds / abs(g)
    ze, zte = np.einsum("nkl,nl->nk", Z, e), np.einsum("nlk,nl->nk", Z, e)
    # |Z| entry by entry is no unit for an entry of Z that cancels: W = |Mx^-1| (I + |g| |Q| |S|) |Mx^-1| |Q| is what an elimination of
    # [Mx | Q] can lose in each entry (the componentwise condition); it carries the conditioning itself, so no factor kappa beside it
    if gamma == 0:
        aZ = np.abs(Q)
        kz = kappa
    else:
        aMx = eye + abs(g) * np.einsum("nkl,nlm->nkm", np.abs(Q), np.abs(S))                     # the absolute terms that form Mx
        aZ = np.einsum("nij,njk,nkl,nlm->nim", np.abs(Mi), aMx, np.abs(Mi), np.abs(Q))
        kz = np.ones(n, dtype=dtype)
    out = {"kappa": kappa, "det": det}
    out["value"] = logterm + np.einsum("nk,nk->n", e, ze)
    out["A_value"] = a_log + kz * np.einsum("nk,nkl,nl->n", ae, aZ, ae)
    out["dmu"] = ze + zte
    out["A_dmu"] = kz[:, None] * (np.einsum("nkl,nl->nk", aZ, ae) + np.einsum("nlk,nl->nk", aZ, ae))
    out["dsig"] = np.swapaxes(Z, 1, 2) - g * zte[:, :, None] * ze[:, None, :]
    aze, azte = np.einsum("nkl,nl->nk", aZ, ae), np.einsum("nlk,nl->nk", aZ, ae)
    out["A_dsig"] = kz[:, None, None] * (np.swapaxes(aZ, 1, 2) + abs(g) * (azte[:, :, None] * np.abs(ze)[:, None, :] + np.abs(zte)[:, :, None] * aze[:, None, :]))
    out["dsig_sym"] = (out["dsig"] + np.swapaxes(out["dsig"], 1, 2)) / 2
    out["A_dsig_sym"] = (out["A_dsig"] + np.swapaxes(out["A_dsig"], 1, 2)) / 2
    out["dvar"] = np.einsum("nkk->nk", out["dsig"])
    out["A_dvar"] = np.einsum("nkk->nk", out["A_dsig"])
    return out


def state_mp(Q, S, e, gamma, dps=50):
    """One matrix at 50 digits: det, Mx^-1 and Z from mpmath.  Returns the dict of state_terms with mpmath entries (value, dmu, dsig, kappa, det)."""
    import mpmath as mp
    with mp.workdps(dps):
        ds = len(e)
        Qm, Sm = mp.matrix(np.asarray(Q, dtype=np.float64).tolist()), mp.matrix(np.asarray(S, dtype=np.float64).tolist())
        em = mp.matrix([v if isinstance(v, mp.mpf) else mp.mpf(float(v)) for v in e])
        g = mp.mpf(float(gamma))
        if gamma == 0:
            Z, det, kappa = Qm, mp.mpf(1), mp.mpf(1)
            logterm = sum(Qm[k, l] * Sm[l, k] for k in range(ds) for l in range(ds))
        else:
            Mx = mp.eye(ds) + g * Qm * Sm
            det, Mi = mp.det(Mx), mp.inverse(Mx)
            Z = Mi * Qm
            kappa = mp.mnorm(Mx, mp.inf) * mp.mnorm(Mi, mp.inf)
            logterm = mp.log(det) / g if det > 0 else mp.nan
        ze, zte = Z * em, Z.T * em
        return {"value": logterm + (em.T * ze)[0], "dmu": [ze[k] + zte[k] for k in range(ds)],
                "dsig": [[Z[l, k] - g * zte[k] * ze[l] for l in range(ds)] for k in range(ds)], "kappa": kappa, "det": det}


def state_value_mp(Q, S, mu, xref, gamma, dps=50):
    """The reference's expression itself at 50 digits (inverse of Q, inverse of Q^-1 + g S): what the central differences are taken of."""
    import mpmath as mp
    with mp.workdps(dps):
        ds = Q.rows
        e = mu - xref
        return mp.log(mp.det(mp.eye(ds) + gamma * Q * S)) / gamma + (e.T * mp.inverse(mp.inverse(Q) + gamma * S) * e)[0]


def input_terms(U, R, Rd=None, last_u=None, uref=None, dtype=LD, defect=None):
    """U [B][H][da]; R, Rd [da][da] general; uref [da] or [H][da] (a schedule's rows).  value [B], dU [B][H][da] and their units.
    defect (float64 emulations of test_host_cost): 'no_neighbour' drops the -(R_d + R_d^T)(u_j+1 - u_j) part of d/du_j, 'no_last_u' takes
    u_-1 = 0."""
    U = np.asarray(U, dtype=dtype)
    B, H, da = U.shape
    R = np.asarray(R, dtype=dtype).reshape(da, da)
    ur = np.zeros(da, dtype=dtype) if uref is None else np.asarray(uref, dtype=dtype)
    d = U - ur
    ad, aR = np.abs(d), np.abs(R)
    out = {"value": np.einsum("bhk,kl,bhl->b", d, R, d), "A_value": np.einsum("bhk,kl,bhl->b", ad, aR, ad),
           "dU": np.einsum("kl,bhl->bhk", R, d) + np.einsum("lk,bhl->bhk", R, d),
           "A_dU": np.einsum("kl,bhl->bhk", aR, ad) + np.einsum("lk,bhl->bhk", aR, ad)}
    if Rd is not None and da > 0:
        Rd = np.asarray(Rd, dtype=dtype).reshape(da, da)
        lu = np.zeros(da, dtype=dtype) if last_u is None or defect == "no_last_u" else np.asarray(last_u, dtype=dtype)
        prev = np.concatenate([np.broadcast_to(lu, (B, 1, da)), U[:, :-1]], axis=1)
        dd = U - prev
        add, aRd = np.abs(dd), np.abs(Rd)
        out["value"] = out["value"] + np.einsum("bhk,kl,bhl->b", dd, Rd, dd)
        out["A_value"] = out["A_value"] + np.einsum("bhk,kl,bhl->b", add, aRd, add)
        gd = np.einsum("kl,bhl->bhk", Rd, dd) + np.einsum("lk,bhl->bhk", Rd, dd)
        agd = np.einsum("kl,bhl->bhk", aRd, add) + np.einsum("lk,bhl->bhk", aRd, add)
        dU, A = out["dU"] + gd, out["A_dU"] + agd
        if defect != "no_neighbour":
            dU[:, :-1] -= gd[:, 1:]
        A[:, :-1] += agd[:, 1:]
        out["dU"], out["A_dU"] = dU, A
    return out


def schedule_rows(H, ds, x_ref=None, X_ref=None, Q=None, Q_f=None, defect=None):
    """Per-step references [H+1][ds] and weights [H+1][ds][ds] of a call: row i of X_ref, Q_f at step H only and only where one is set.
    defect 'qf_early': Q_f at step H - 1."""
    xr = np.broadcast_to(np.zeros(ds) if x_ref is None else np.asarray(x_ref), (H + 1, ds)) if X_ref is None else np.asarray(X_ref)[:H + 1]
    Qs = np.broadcast_to(np.asarray(Q), (H + 1, ds, ds)).copy()
    if Q_f is not None:
        Qs[H - 1 if defect == "qf_early" else H] = Q_f
    return xr, Qs


def cost_terms(means, covs, U, gamma, Q, R, Rd=None, last_u=None, x_ref=None, u_ref=None, X_ref=None, U_ref=None, Q_f=None, dtype=LD):
    """A whole call: means [B][H+1][ds], covs [B][H+1][ds][ds], U [B][H][da].  Dict: value [B] and A_value, dmu, dsig, dsig_sym, dvar with
    their units ([B][H+1]...), dU and A_dU, kappa and det [B][H+1], value_state [B][H+1], value_input [B]."""
    means = np.asarray(means)
    B, H1, ds = means.shape
    H = H1 - 1
    xr, Qs = schedule_rows(H, ds, x_ref, X_ref, Q, Q_f)
    e = np.asarray(means, dtype=dtype) - np.asarray(xr, dtype=dtype)
    st = state_terms(np.broadcast_to(Qs, (B, H1, ds, ds)).reshape(B * H1, ds, ds), np.asarray(covs).reshape(B * H1, ds, ds),
                     e.reshape(B * H1, ds), gamma, dtype)
    out = {k: v.reshape((B, H1) + v.shape[1:]) for k, v in st.items()}
    inp = input_terms(U, R, Rd, last_u, u_ref if U_ref is None else np.asarray(U_ref)[:H], dtype)
    out["value_state"], out["A_value_state"], out["value_input"] = out["value"], out["A_value"], inp["value"]
    out["value"] = out["value_state"].sum(1) + inp["value"]
    out["A_value"] = out["A_value"].sum(1) + inp["A_value"]
    out["dU"], out["A_dU"] = inp["dU"], inp["A_dU"]
    return out


def sweep(J, g_means=None, g_vars=None, dtype=LD, defect=None):
    """Reverse sweep over J [B][H][2ds][2ds+da] (rows mu_t, var_t; columns mu_t-1, var_t-1, u_t-1) with upstream seeds g_means, g_vars
    [B][H+1][ds] at EVERY step, either absent: gU [B][H][da], gx0 [B][ds].  defect 'drop_seed': the seeds of the steps before H are dropped."""
    J = np.asarray(J, dtype=dtype)
    B, H, nz, nc = J.shape
    ds = nz // 2

    def seed(t):
        a = np.zeros((B, nz), dtype=dtype)
        if defect == "drop_seed" and t < H:
            return a
        if g_means is not None:
            a[:, :ds] = np.asarray(g_means, dtype=dtype)[:, t]
        if g_vars is not None:
            a[:, ds:] = np.asarray(g_vars, dtype=dtype)[:, t]
        return a
    adj = seed(H)
    gU = np.zeros((B, H, nc - nz), dtype=dtype)
    for t in range(H, 0, -1):
        s = np.einsum("brc,br->bc", J[:, t - 1], adj)
        gU[:, t - 1] = s[:, nz:]
        adj = seed(t - 1) + s[:, :nz]
    return gU, adj[:, :ds]


def sweep_unit(J, a_means=None, a_vars=None, dtype=LD):
    """The same sweep over |J| and the |seeds| (or the units of the seeds): the error unit of gU and gx0."""
    ab = lambda a: None if a is None else np.abs(np.asarray(a, dtype=dtype))  # noqa: E731
    return sweep(np.abs(np.asarray(J, dtype=dtype)), ab(a_means), ab(a_vars), dtype)


def k_of(got, ref, A):
    """Worst K = |got - ref| / (2^-53 A) over the entries; an entry whose unit is 0 must be exact."""
    got, ref, A = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD), np.asarray(A, dtype=LD)
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    assert np.all(np.isfinite(err)), "non-finite entries"
    assert np.all(err[A == 0] == 0), "an entry with a zero unit is not exact"
    return float(np.max(np.where(A > 0, err / (U53 * np.where(A > 0, A, 1)), 0)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the four eliminations as the kernels write them, float64
# ---------------------------------------------------------------------------------------------------------------------------------------
def emulate(form, Q, S, e, gamma, defect=None):
    """Float64 emulation of state_cost ('full'), state_cost_sched ('sched': the same arithmetic, the swap as predicated moves),
    state_cost_diag ('diag': S [n][ds] variances, Mx = I + g (Q_rc var_c)) and fc_state_cost ('fc': compare-and-swap of row k with every
    later row in turn, symmetrised d/dS).  Multiply and add where the kernels fuse them.  Returns value, dmu, dsig ('diag': dvar), and what
    the pivoting did: swaps [n][ds] row exchanges per column, margin [n] the smallest ratio of the two sides of any pivot comparison that
    decided something (the winner against the runner-up; for the cascade every comparison made).
    defect: 'no_sign' | 'swap_left' | 'no_fabs' | 'z_for_zt' (test_host_cost)."""
    assert form in FORMS
    S = np.asarray(S, dtype=np.float64)
    n, ds = S.shape[0], S.shape[1]
    Q = np.ascontiguousarray(np.broadcast_to(np.asarray(Q, dtype=np.float64), (n, ds, ds)))
    e = np.asarray(e, dtype=np.float64)
    g = float(gamma)
    swaps = np.zeros((n, ds), dtype=int)
    margin = np.full(n, np.inf)
    idx = np.arange(n)
    if g == 0.0:
        Z = Q
        if form == "diag":
            c = np.einsum("nkk,nk->n", Q, S)
        else:
            c = np.einsum("nkl,nlk->n", Q, S)
        det = None
    else:
        if form == "diag":
            QS = Q * S[:, None, :]
        else:
            QS = np.zeros((n, ds, ds))
            for l in range(ds):
                QS = QS + Q[:, :, l, None] * S[:, l, None, :]
        w = np.concatenate([np.eye(ds)[None] + g * QS, Q], axis=2)
        ncol = ds if defect == "swap_left" else 2 * ds
        key = (lambda a: a) if defect == "no_fabs" else np.abs
        det = np.ones(n)
        for k in range(ds):
            if form == "fc":
                for r in range(k + 1, ds):
                    a, b = key(w[:, r, k]), key(w[:, k, k])
                    sw = a > b
                    hi, lo = np.maximum(np.abs(a), np.abs(b)), np.minimum(np.abs(a), np.abs(b))
                    with np.errstate(divide="ignore", invalid="ignore"):
                        margin = np.minimum(margin, np.where(lo > 0, hi / lo, np.inf))
                    rk, rr = w[:, k, :ncol].copy(), w[:, r, :ncol].copy()
                    w[:, k, :ncol] = np.where(sw[:, None], rr, rk)
                    w[:, r, :ncol] = np.where(sw[:, None], rk, rr)
                    swaps[:, k] += sw
                    if defect != "no_sign":
                        det = np.where(sw, -det, det)
            elif k + 1 < ds:
                col = key(w[:, k:, k])
                piv = np.argmax(col, axis=1)                      # (the first of equal entries, like the kernels' strict >)
                srt = np.sort(np.abs(col), axis=1)
                with np.errstate(divide="ignore", invalid="ignore"):
                    margin = np.minimum(margin, np.where(srt[:, -2] > 0, srt[:, -1] / srt[:, -2], np.inf))
                sw = piv > 0
                rk, rp = w[idx, k, :ncol].copy(), w[idx, k + piv, :ncol].copy()
                w[idx, k + piv, :ncol] = rk
                w[idx, k, :ncol] = rp
                swaps[:, k] += sw
                if defect != "no_sign":
                    det = np.where(sw, -det, det)
            pv = w[:, k, k].copy()
            det = det * pv
            w[:, k, :] = w[:, k, :] * (1.0 / pv)[:, None]
            for r in range(ds):
                if r != k:
                    w[:, r, :] = w[:, r, :] - w[:, r, k, None] * w[:, k, :]
        Z = w[:, :, ds:]
    ze, zte, quad = np.zeros((n, ds)), np.zeros((n, ds)), np.zeros(n)
    for k in range(ds):
        for l in range(ds):
            ze[:, k] += Z[:, k, l] * e[:, l]
            zte[:, k] += Z[:, l, k] * e[:, l]
        quad += e[:, k] * ze[:, k]
    with np.errstate(invalid="ignore", divide="ignore"):
        value = (c if g == 0.0 else np.log(det) / g) + quad
    Zt = Z if defect == "z_for_zt" else np.swapaxes(Z, 1, 2)
    dsig = Zt - g * zte[:, :, None] * ze[:, None, :]
    if form == "fc":
        dsig = 0.5 * (dsig + np.swapaxes(dsig, 1, 2))
    out = {"value": value, "dmu": ze + zte, "swaps": swaps, "margin": margin, "det": det}
    if form == "diag":
        out["dvar"] = np.einsum("nkk->nk", dsig).copy()
    else:
        out["dsig"] = dsig
    return out


def emulate_terms(form, means, covs, gamma, Q, x_ref=None, X_ref=None, Q_f=None, defect=None):
    """emulate() over a call: means [B][H+1][ds], covs [B][H+1][ds][ds] ('diag': vars [B][H+1][ds]); entries reshaped to [B][H+1]...;
    value_state [B][H+1]."""
    means = np.asarray(means, dtype=np.float64)
    B, H1, ds = means.shape
    xr, Qs = schedule_rows(H1 - 1, ds, x_ref, X_ref, Q, Q_f, defect if defect == "qf_early" else None)
    covs = np.asarray(covs, dtype=np.float64)
    em = emulate(form, np.broadcast_to(Qs, (B, H1, ds, ds)).reshape(B * H1, ds, ds), covs.reshape((B * H1,) + covs.shape[2:]),
                 (means - xr).reshape(B * H1, ds), gamma, None if defect == "qf_early" else defect)
    out = {k: v.reshape((B, H1) + v.shape[1:]) for k, v in em.items() if v is not None}
    out["value_state"] = out.pop("value")
    return out


def swap_summary(swaps):
    """swaps [...][ds] -> (columns that swapped somewhere, a slot with an odd total, a slot with an even total >= 2, a column with > 1)."""
    s = swaps.reshape(-1, swaps.shape[-1])
    tot = s.sum(1)
    return set(np.nonzero(s.sum(0))[0].tolist()), bool(np.any(tot % 2 == 1)), bool(np.any((tot % 2 == 0) & (tot >= 2))), bool(np.any(s > 1))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the input tables
# ---------------------------------------------------------------------------------------------------------------------------------------
def spectral_radius(Q, S):
    return np.array([np.abs(np.linalg.eigvals(q @ s)).max() for q, s in zip(np.broadcast_to(Q, S.shape), S)])


def gen_Q(rng, ds):
    A = rng.standard_normal((ds, ds))
    return A @ A.T / ds + 0.3 * np.eye(ds) + 0.1 * rng.standard_normal((ds, ds))


def gen_R(rng, da):
    A = rng.standard_normal((da, da))
    return A @ A.T / max(da, 1) + 0.2 * np.eye(da) + 0.1 * rng.standard_normal((da, da))


def gen_call(seed, ds, da, H, B, family="neg", diag=False, sched=False, q_f=False):
    """One call of the tables.  Q = A A^T / ds + 0.3 I + a 0.1 non-symmetric perturbation; every slot S = B B^T / ds + 0.05 I + a 0.02
    non-symmetric perturbation (diag: var ~ U(0.3, 3)), scaled so that rho(Q S) of the slot is r times the largest of the call, r = 1 for one
    slot in four, U(0.55, 1) for half of them and U(0.02, 0.3) for the rest: many slots close to the edge and some near the identity;
    gamma = -0.9 / max rho ('neg'), 3 / max rho ('pos'), 0 ('zero'); 'tiny': see below.  Non-symmetric R and R_delta, a non-zero last_u; with `sched` rows
    X_ref [H+1][ds], U_ref [H][da] and, with `q_f`, a terminal weight from the same generator as Q (so step H pivots under ITS weight:
    rho is taken with the weight of each slot)."""
    rng = np.random.default_rng([seed, ds, da, H, B, FORMS.index("diag") if diag else 0, {"neg": 0, "pos": 1, "zero": 2, "tiny": 3}[family]])
    Q = gen_Q(rng, ds)
    Q_f = gen_Q(rng, ds) if q_f else None
    n = B * (H + 1)
    if diag:
        S = np.stack([np.diag(v) for v in rng.uniform(0.3, 3.0, (n, ds))])
    else:
        Bm = rng.standard_normal((n, ds, ds))
        S = Bm @ np.swapaxes(Bm, 1, 2) / ds + 0.05 * np.eye(ds) + 0.02 * rng.standard_normal((n, ds, ds))
    Qs = np.broadcast_to(Q, (B, H + 1, ds, ds)).copy()
    if q_f:
        Qs[:, H] = Q_f
    rho = spectral_radius(Qs.reshape(n, ds, ds), S)
    pick = rng.uniform(size=n)
    r = np.where(pick < 0.25, 1.0, np.where(pick < 0.75, rng.uniform(0.55, 1.0, n), rng.uniform(0.02, 0.3, n)))
    r[rng.integers(n)] = 1.0
    S = S * (r / rho)[:, None, None] * np.median(rho)
    rho_max = float((r * np.median(rho)).max())
    if family == "tiny":
        # one slot whose leading entry 1 + gamma (Q S)_00 is 1e-6 while the entries below it are of order one -- an elimination that pivots on
        # it loses six digits --, the others scaled back inside gamma rho = -0.9; the caller keeps the seeds whose determinants are positive
        j = int(np.argmax(r))
        gamma = -(1.0 - 1e-6) / (Qs.reshape(n, ds, ds)[j] @ S[j])[0, 0]
        rs = r * np.median(rho)
        S = S * np.where(np.arange(n) == j, 1.0, np.minimum(1.0, 0.9 / (abs(gamma) * rs)))[:, None, None]
    else:
        gamma = {"neg": -0.9 / rho_max, "pos": 3.0 / rho_max, "zero": 0.0}[family]
    c = dict(ds=ds, da=da, H=H, B=B, family=family, gamma=gamma, Q=Q, Q_f=Q_f, rho_max=rho_max,
             means=rng.standard_normal((B, H + 1, ds)), covs=S.reshape(B, H + 1, ds, ds),
             U=rng.standard_normal((B, H, da)), R=gen_R(rng, da), Rd=gen_R(rng, da), last_u=rng.standard_normal(da),
             x_ref=0.5 * rng.standard_normal(ds), u_ref=0.5 * rng.standard_normal(da), X_ref=None, U_ref=None)
    if diag:
        c["vars"] = np.einsum("bhkk->bhk", c["covs"]).copy()
    if sched:
        c["X_ref"], c["U_ref"] = 0.5 * rng.standard_normal((H + 1, ds)), 0.5 * rng.standard_normal((H, da))
    return c


def call_kwargs(c):
    return dict(gamma=c["gamma"], Q=c["Q"], R=c["R"], Rd=c["Rd"], last_u=c["last_u"], x_ref=c["x_ref"], u_ref=c["u_ref"],
                X_ref=c["X_ref"], U_ref=c["U_ref"], Q_f=c["Q_f"])


# seeds chosen (as the conditions of test_host_cost.py allow) where twelve draws leave a condition open: a swap in column 0 at ds = 7, 8 and a
# condition number above 30 with a diagonal Sigma at ds = 2, 3, 4, 6
EXTRA_SEEDS = {(7, False): [16], (8, False): [14], (2, True): [208], (3, True): [115], (4, True): [132], (6, True): [135]}


# seeds of the 'tiny' family chosen from the REFERENCE side: determinants above 1e-3, kappa below 300, no pivot comparison closer than 1.001,
# K_ref below 30, and every entry below the tiny one negative, so that an elimination choosing its pivot without fabs takes the tiny one
# (the float64 emulation of that defect then lies more than 100 K_ref away)
TINY_SEEDS = {(2, False): [5, 23], (3, False): [19, 48], (4, False): [45, 60], (5, False): [7, 20], (6, False): [69, 92], (7, False): [569, 580],
              (8, False): [368, 958], (2, True): [46, 92], (3, True): [2, 7], (4, True): [24, 76], (5, True): [44, 71], (6, True): [39, 184],
              (7, True): [258, 359], (8, True): [665, 720]}


def gen_vjp(seed, ds, da, H, B):
    """Random step Jacobians [B][H][2ds][2ds+da] of unit row scale and seeds at every step, for the reverse sweep."""
    rng = np.random.default_rng([seed, ds, da, H, B, 77])
    nz, nc = 2 * ds, 2 * ds + da
    return dict(J=rng.standard_normal((B, H, nz, nc)) / np.sqrt(nz), gm=rng.standard_normal((B, H + 1, ds)), gv=rng.standard_normal((B, H + 1, ds)))


def host_table(ds, diag=False):
    """The calls test_host_cost.py asserts the input conditions on, per state dimension: twelve pivoting calls of 16 slots (every fourth with
    a schedule and a terminal weight) and the chosen seeds above, a well-conditioned gamma > 0 call and a gamma = 0 call."""
    t = [gen_call(s, ds, 2, 7, 2, "neg", diag=diag, sched=s % 4 == 3 and s < NEG_CALLS, q_f=s % 4 == 3 and s < NEG_CALLS)
         for s in list(range(NEG_CALLS)) + EXTRA_SEEDS.get((ds, diag), [])]
    t += [gen_call(s, ds, 2, 7, 2, "tiny", diag=diag) for s in TINY_SEEDS[ds, diag]]
    return t + [gen_call(0, ds, 2, 7, 2, "pos", diag=diag), gen_call(0, ds, 2, 7, 2, "zero", diag=diag)]


# The absolute caps of tests/test_gpu_cost.py per (form, output): twice the worst K measured on an MI355X
CAP_K = {("full", "value"): 4.7, ("full", "dmu"): 7.1, ("full", "dsig"): 7.3, ("sched", "value"): 6.1, ("sched", "dmu"): 6.7,
         ("sched", "dsig"): 8.3, ("input_cost", "dU"): 5.9, ("k_rollout_vjp", "gU"): 4.3, ("k_rollout_vjp", "gx0"): 4.1,
         ("state_cost_diag", "value"): 1.3, ("tail sweep, all in LDS", "grad"): 0.94, ("tail sweep, streaming", "grad"): 1.4,
         ("fc_state_cost", "value"): 2.3}
# relative error of the cost and (in norm) of the gradient of k_fc_tail against the long double complex step: twice the worst measured
CAP_REL = {"fc cost": 2.7e-14, "fc grad": 7.8e-14}


def k_state(form, em, ref):
    """K per output of an emulation (or of kernel outputs laid out like one) against the reference terms of the same call."""
    out = {"value": k_of(em["value_state"], ref["value_state"], ref["A_value_state"]) if "A_value_state" in ref else None,
           "dmu": k_of(em["dmu"], ref["dmu"], ref["A_dmu"])}
    if form == "diag":
        out["dvar"] = k_of(em["dvar"], ref["dvar"], ref["A_dvar"])
    elif form == "fc":
        out["dsig"] = k_of(em["dsig"], ref["dsig_sym"], ref["A_dsig_sym"])
    else:
        out["dsig"] = k_of(em["dsig"], ref["dsig"], ref["A_dsig"])
    return out
