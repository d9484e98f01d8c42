"""Extended-precision restatement of the commanded input under a linear state feedback, u_t = v_t + K_t (x_t - mu_t) ~ N(v_t, K_t Sigma_t
K_t^T) (gpmpc_feedback_input_cost, gpmpc_feedback_input_constraints, gpmpc_particle_inputs; include/gpmpc.h, "Linearised propagation,
full covariance: the commanded input").  TEST INFRASTRUCTURE ONLY.

Conventions of tests/linprop_fc_reference.py: ``np.longdouble``, the float64 inputs are data, every sum comes back with the sum of the
absolute values of its terms (the unit of the bound 1e-12 sum |terms|), structural zeros have a zero unit.

    input cost          c = sum_{j<H} sum_{a,b,k,l} R_ab K_bk Sigma_j[k][l] K_al;    d c / d Sigma_j[k][l] = sum_{a,b} K_al R_ab K_bk, 0 at j = H
    input constraints   a = K_t^T c_r,  q = a^T Sigma_t a,  sd = sqrt(q) (0 where q <= 0),  g_u[t][r] = c_r . v_t + kappa_r sd - d_r
                        Jacobian [H m][H da]:  tau > t: 0;  tau = t: c_rj;  tau < t: kappa / (2 sd) sum_{k<=l} w_kl S_t[Sigma_kl][tau, j],
                        w_kk = a_k^2, w_kl = 2 a_k a_l; S_t: the sensitivities of the packed state of step t, S_0 = 0
    units               q: the terms of the full expansion, (|K|^T |c|)^T |Sigma| (|K|^T |c|); g_u: |c| . |v| + |d| + kappa (sd + q_abs / (2 sd));
                        the Jacobian: as linprop_fc_reference.constraints, S carried through |J|, the weights with the units of a

Keyword switches for deliberate MISTAKES (the discriminating controls):
    offdiag_once         weight a_k a_l instead of 2 a_k a_l for k < l                        (the Jacobian)
    gain_of_next_step    K_{t+1} where K_t belongs (the last step keeps its own)              (cost, seed, values, Jacobian)
    cov_after_step       Sigma_{t+1} (and S_{t+1}) where Sigma_t belongs                      (cost, values, Jacobian)
    R_transposed         R^T in the seed: sum_{a,b} K_al R_ba K_bk                            (the seed)
"""
import numpy as np

import gpstate_reference as G
import linprop_fc_reference as F

LD = G.LD


def gains(K, H, ds, da, dtype=LD, shift=False):
    """(H, da, ds) from None (zeros), (da, ds) or (H, da, ds); shift: the gain of the next step, the last one kept."""
    if K is None:
        return np.zeros((H, da, ds), dtype=dtype)
    K = np.asarray(K, dtype=dtype)
    Kh = np.broadcast_to(K, (H, da, ds)).copy() if K.ndim == 2 else K.copy()
    if shift:
        Kh = np.concatenate([Kh[1:], Kh[-1:]], axis=0)
    return Kh


def input_cov(covs, K, dtype=LD):
    """K_t Sigma_t K_t^T, (B, H, da, da), from covs (B, H+1, ds, ds)."""
    covs = np.asarray(covs, dtype=dtype)
    B, H1, ds, _ = covs.shape
    Kh = gains(K, H1 - 1, ds, np.asarray(K).shape[-2], dtype)
    return np.einsum("tik,btkl,tjl->btij", Kh, covs[:, :-1], Kh)


def input_cost(covs, K, Rm, dtype=LD, gain_of_next_step=False, cov_after_step=False, R_transposed=False):
    """dict(c, A_c (B,), dcovs, A_dcovs (B, H+1, ds, ds))."""
    covs = np.asarray(covs, dtype=dtype)
    B, H1, ds, _ = covs.shape
    H = H1 - 1
    Rm = np.asarray(Rm, dtype=dtype)
    da = Rm.shape[0]
    Kh = gains(K, H, ds, da, dtype, shift=gain_of_next_step)
    S = covs[:, 1:] if cov_after_step else covs[:, :-1]
    M = np.einsum("tal,ab,tbk->tkl", Kh, Rm, Kh)                              # d c / d Sigma_t[k][l]
    Ma = np.einsum("tal,ab,tbk->tkl", np.abs(Kh), np.abs(Rm), np.abs(Kh))
    Ms = np.einsum("tal,ba,tbk->tkl", Kh, Rm, Kh) if R_transposed else M
    dc, dca = np.zeros((B, H1, ds, ds), dtype=dtype), np.zeros((B, H1, ds, ds), dtype=dtype)
    dc[:, :H], dca[:, :H] = Ms[None], Ma[None]
    return {"c": np.einsum("tkl,btkl->b", M, S), "A_c": np.einsum("tkl,btkl->b", Ma, np.abs(S)), "dcovs": dc, "A_dcovs": dca}


def sensitivities(jac, dtype=LD, jac_units=None):
    """S, Sa (H+1, B, p, H da): the sensitivities of the packed state of every step by the inputs, and the same through |J| (or through
    ``jac_units`` >= |J|, where the Jacobians themselves carry an error: |J| + E / tol makes tol Sa cover it to first order and beyond)."""
    J = np.asarray(jac, dtype=dtype)
    Ja = np.abs(J) if jac_units is None else np.asarray(jac_units, dtype=dtype)
    B, H, p, nc = J.shape
    da = nc - p
    S, Sa = [np.zeros((B, p, H * da), dtype=dtype)], [np.zeros((B, p, H * da), dtype=dtype)]
    for t in range(H):
        s, sa = np.einsum("brk,bkc->brc", J[:, t, :, :p], S[-1]), np.einsum("brk,bkc->brc", Ja[:, t, :, :p], Sa[-1])
        s[:, :, t * da:(t + 1) * da], sa[:, :, t * da:(t + 1) * da] = J[:, t, :, p:], Ja[:, t, :, p:]
        s[:, :, (t + 1) * da:], sa[:, :, (t + 1) * da:] = 0, 0
        S.append(s)
        Sa.append(sa)
    return np.stack(S), np.stack(Sa)


def input_constraints(U, covs, jac, K, C, d, kappa, dtype=LD, jac_units=None, offdiag_once=False, gain_of_next_step=False,
                      cov_after_step=False):
    """U (B, H, da), covs (B, H+1, ds, ds), jac (B, H, p, p + da) or None (values only), rows C (m, da), d, kappa (m,).
    dict(g, A_g (B, H, m), sd, q; gjac, A_gjac (B, H m, H da))."""
    U, covs = np.asarray(U, dtype=dtype), np.asarray(covs, dtype=dtype)
    C, d, kappa = np.atleast_2d(np.asarray(C, dtype=dtype)), np.asarray(d, dtype=dtype).reshape(-1), np.asarray(kappa, dtype=dtype).reshape(-1)
    B, H, da = U.shape
    ds, m = covs.shape[2], C.shape[0]
    Kh = gains(K, H, ds, da, dtype, shift=gain_of_next_step)
    off = 1 if cov_after_step else 0
    Sg = covs[:, off:off + H]
    a = np.einsum("rj,tjk->trk", C, Kh)                                        # (H, m, ds)
    aa = np.einsum("rj,tjk->trk", np.abs(C), np.abs(Kh))
    cm, cm_abs = np.einsum("rj,btj->btr", C, U), np.einsum("rj,btj->btr", np.abs(C), np.abs(U))
    q, q_abs = np.einsum("trk,btkl,trl->btr", a, Sg, a), np.einsum("trk,btkl,trl->btr", aa, np.abs(Sg), aa)
    pos = q > 0
    sd = np.where(pos, np.sqrt(np.where(pos, q, 1)), 0)
    out = {"g": cm + kappa[None, None, :] * sd - d[None, None, :], "sd": sd, "q": q,
           "A_g": cm_abs + np.abs(d)[None, None, :] + kappa[None, None, :] * (sd + np.where(pos, q_abs / (2 * np.where(pos, sd, 1)), 0))}
    if jac is None:
        return out
    S, Sa = sensitivities(jac, dtype, jac_units)
    pairs = F.tri_pairs(ds)
    w = np.stack([a[:, :, k] * a[:, :, l] * (1 if (k == l or offdiag_once) else 2) for k, l in pairs], axis=2)      # (H, m, nt)
    wa = np.stack([aa[:, :, k] * aa[:, :, l] * (1 if k == l else 2) for k, l in pairs], axis=2)
    f = np.where(pos, kappa[None, None, :] / (2 * np.where(pos, sd, 1)), 0)
    gj, gja = np.zeros((B, H * m, H * da), dtype=dtype), np.zeros((B, H * m, H * da), dtype=dtype)
    for t in range(H):
        St, Sat = S[t + off][:, ds:], Sa[t + off][:, ds:]
        dv = np.einsum("rv,bvc->brc", w[t], St)
        dva = np.einsum("rv,bvc->brc", wa[t], np.abs(St)) + np.einsum("rv,bvc->brc", np.abs(w[t]), Sat)
        ft = f[:, t, :, None]
        rel = np.where(pos[:, t], q_abs[:, t] / np.where(pos[:, t], q[:, t], 1), 0)[:, :, None]
        blk, blka = ft * dv, np.abs(ft) * dva + np.abs(ft * dv) * (1 + rel)
        blk[:, :, t * da:], blka[:, :, t * da:] = 0, 0                         # tau >= t: no variance part (exact)
        blk[:, :, t * da:(t + 1) * da] = C[None]                               # tau = t: the direct part, exact
        gj[:, t * m:(t + 1) * m], gja[:, t * m:(t + 1) * m] = blk, blka
    out.update(gjac=gj, A_gjac=gja)
    return out


# ---------------------------------------------------------------------------------------------------------------- particles
def particle_inputs(x, v, K, mu, dtype=LD):
    """u^p = v_b + K (x^p - mu_b): x (B, P, ds), v (B, da), K (da, ds) or None, mu (B, ds) -> u, A_u (B, P, da)."""
    x, v, mu = np.asarray(x, dtype=dtype), np.asarray(v, dtype=dtype), np.asarray(mu, dtype=dtype)
    B, P, ds = x.shape
    if K is None:
        u = np.broadcast_to(v[:, None, :], (B, P, v.shape[1])).copy()
        return u, np.abs(u)
    K = np.asarray(K, dtype=dtype)
    e = x - mu[:, None, :]
    return v[:, None, :] + np.einsum("jk,bpk->bpj", K, e), np.abs(v)[:, None, :] + np.einsum("jk,bpk->bpj", np.abs(K), np.abs(x) + np.abs(mu)[:, None, :])
