"""Extended-precision restatement of the particle cost (gpmpc_particle_cost, gpmpc_particle_evaluate, gpmpc_mppi_solve_particles;
include/gpmpc.h, "Particle cost").  TEST INFRASTRUCTURE ONLY.

    J_b = sum_{i = 0...H} s_i + input_cost(U_b)
    c_p = e_p^T Q_i e_p,  e_p = x_i^p - x_ref,i
    gamma == 0:  s_i = (1 / P) sum_p c_p
    otherwise:   a_p = -(gamma / 2) c_p,  M = max_p a_p,  s_i = -(2 / gamma) (M + log((1 / P) sum_p exp(a_p - M)))
    rows:        y_p = a_r . x_t^p - b_r sorted ascending,  eps_r = 1/2 erfc(kappa_r / sqrt 2),  m_r = floor(eps_r P + 1e-9),
                 g[t-1][r] = y_(P - m_r)            (numpy's sort; the library selects in LDS)

``numpy.longdouble`` throughout, none of the kernel's groupings (no strided partial sums, no folds); the per-step reference and weight come
from ``cost_reference.schedule_rows`` and the input terms from ``cost_reference.input_terms``, the yardsticks of the cost kernels.  Beside
every value stands the sum of absolute terms the GPU tests scale their rounding budget with.  The keyword arguments ``gamma_sign``,
``mean_only`` and ``index_shift`` are deliberate MISTAKES for the discriminating controls.

Composes with ``particle_reference.rollout`` (``evaluate``) and, through that, with ``mppi_reference.solve``."""
import math

import numpy as np

import cost_reference as CR

LD = np.longdouble


def quantile_counts(kappa, P):
    """m_r = floor(eps_r P + 1e-9), eps_r = 1/2 erfc(kappa_r / sqrt 2): how many of P particles may violate row r (host, double)."""
    return np.array([int(math.floor(0.5 * math.erfc(float(k) / math.sqrt(2.0)) * P + 1e-9)) for k in np.atleast_1d(kappa)], dtype=np.int64)


def stage(X, Q, xref, gamma, gamma_sign=1.0, mean_only=False):
    """X (..., P, ds), Q (ds, ds) as given, xref (ds,): dict(value (...), c (..., P), c_abs (..., P) = sum_kl |e_k| |Q_kl| |e_l|).
    A NaN coordinate in any particle makes the value NaN."""
    X = np.asarray(X, dtype=np.float64)
    P = X.shape[-2]
    e = X.astype(LD) - np.asarray(xref, dtype=LD)
    Ql = np.asarray(Q, dtype=LD)
    c = np.einsum("...k,kl,...l->...", e, Ql, e)
    c_abs = np.einsum("...k,kl,...l->...", np.abs(e), np.abs(Ql), np.abs(e))
    g = LD(gamma) * LD(gamma_sign)
    if gamma == 0 or mean_only:
        value = c.sum(axis=-1) / LD(P)
    else:
        a = -(g / 2) * c
        with np.errstate(invalid="ignore"):
            M = a.max(axis=-1)
            value = -(2 / g) * (M + np.log(np.exp(a - M[..., None]).sum(axis=-1) / LD(P)))
    bad = np.isnan(X).any(axis=(-1, -2))
    value = np.where(bad, LD("nan"), value)
    return {"value": value, "c": c, "c_abs": c_abs}


def rows(X, A, b, kappa, index_shift=0):
    """X (..., P, ds): dict(g (..., rows) = y_(P - m_r), unit (..., rows) = max_p sum_k |a_rk x_k| + |b_r|, m (rows,)).  An order statistic is
    1-Lipschitz in the sup norm of the margins, so a bound on every margin's error is a bound on g's."""
    X = np.asarray(X, dtype=np.float64)
    P = X.shape[-2]
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    m = quantile_counts(np.broadcast_to(np.asarray(kappa, dtype=np.float64).reshape(-1), (A.shape[0],)), P)
    y = np.einsum("...pk,rk->...rp", X.astype(LD), A.astype(LD)) - b.astype(LD)[:, None]
    unit = np.einsum("...pk,rk->...rp", np.abs(X).astype(LD), np.abs(A).astype(LD)).max(axis=-1) + np.abs(b).astype(LD)
    bad = np.isnan(X).any(axis=(-1, -2))
    ys = np.sort(np.where(bad[..., None, None], LD(0), y), axis=-1)
    idx = np.clip(P - m - 1 + index_shift, 0, P - 1)                      # 0-based index of y_(P - m_r)
    g = np.stack([ys[..., r, idx[r]] for r in range(A.shape[0])], axis=-1)
    g = np.where(bad[..., None], LD("nan"), g)
    return {"g": g, "unit": unit, "m": m}


def cost(X, U, gamma, Q, R, Rd=None, last_u=None, x_ref=None, u_ref=None, X_ref=None, U_ref=None, Q_f=None, cons=None, gamma_sign=1.0,
         mean_only=False, index_shift=0):
    """X (H+1, B, P, ds) (the particles of particle_reference.rollout), U (B, H, da); cons = (A, b, kappa) or None.  Dict:
    cost (B,), stage (B, H+1), c_abs (B, H+1, P), input, A_input (B,) and with cons g, g_unit (B, H, rows), m (rows,)."""
    X = np.asarray(X, dtype=np.float64)
    T, B, P, ds = X.shape
    H = T - 1
    U = np.asarray(U, dtype=np.float64).reshape(B, H, -1)
    xr, Qs = CR.schedule_rows(H, ds, x_ref, X_ref, Q, Q_f)
    st = [stage(X[i], Qs[i], xr[i], gamma, gamma_sign, mean_only) for i in range(T)]
    out = {"stage": np.stack([s["value"] for s in st], axis=1), "c_abs": np.stack([s["c_abs"] for s in st], axis=1),
           "c": np.stack([s["c"] for s in st], axis=1)}
    inp = CR.input_terms(U, R, Rd, last_u, u_ref if U_ref is None else np.asarray(U_ref)[:H])
    out["input"], out["A_input"] = inp["value"], inp["A_value"]
    out["cost"] = out["stage"].sum(axis=1) + inp["value"]
    if cons is not None:
        r = [rows(X[t], cons[0], cons[1], cons[2], index_shift) for t in range(1, T)]
        out["g"], out["g_unit"], out["m"] = np.stack([v["g"] for v in r], axis=1), np.stack([v["unit"] for v in r], axis=1), r[0]["m"]
    return out


def evaluate(model, x0, H, P, seed, call_index, cost_kw, cons=None):
    """U (K, n) -> (cost (K,), g (K, H rows) or None) in float64: the particle reference rolled out from x0 for every plan under the noise
    of (seed, call_index), then ``cost`` -- the ``evaluate`` argument of mppi_reference.solve."""
    import particle_reference as PR
    ds, da, _ = PR.dims(model)

    def run(U):
        K = U.shape[0]
        Ub = np.asarray(U, dtype=np.float64).reshape(K, H, da)
        X, _ = PR.rollout(model, np.tile(np.asarray(x0, dtype=np.float64).reshape(1, ds), (K, 1)), Ub, P, seed=seed, call_index=call_index)
        r = cost(X, Ub, cons=cons, **cost_kw)
        return r["cost"].astype(np.float64), (r["g"].astype(np.float64).reshape(K, -1) if cons is not None else None)
    return run
