"""Float64 CPU reference of the cost with time-varying references and a terminal weight, for tests/test_host_tracking.py and
tests/test_gpu_tracking.py.

Built on the pinned oracle (oracle/gpmpc_oracle.py) and on autograd only -- none of the closed forms of the HIP kernels appear here:

* the trajectory is ``oracle.forward_propagate(..., "o2")`` (``oracle.forward_propagate_fullcov`` for the full-covariance twin, the
  nominal rollout of tests/nominal_reference.py for a pack with a linear nominal model), with ``U.requires_grad_()``;
* the cost is the loop of ``oracle.cost`` / ``oracle.cost_risk_neutral`` written out with ``x_ref[i]``, ``u_ref[j]`` and the weight of
  the step: ``Q_terminal`` at the last step where one is given, ``Q`` elsewhere -- in the log-determinant, the quadratic form and the
  gamma = 0 trace alike;
* the gradient is ``backward()``.
"""
import numpy as np
import torch

from oracle import gpmpc_oracle as O

F64 = torch.float64


def _t(a):
    return a.to(F64) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))


def propagate(gp, horizon, x0, Ut, fullcov=False, nominal=None):
    """Lists of H + 1 means (ds,) and covariances (ds, ds), graph attached to ``Ut``."""
    if nominal is not None:
        from nominal_reference import nominal_step
        W, b = _t(nominal[0]), _t(nominal[1]).reshape(-1)
        resid = gp.Y - gp.X @ W.T - b
        means = [_t(x0).reshape(-1)]
        vars_ = [torch.full((gp.ds,), O.INIT_STATE_VAR, dtype=F64)]
        act_var = torch.full((gp.da,), O.ACTION_NOISE_VAR, dtype=F64)
        for t in range(1, horizon + 1):
            u = torch.cat((means[t - 1], Ut[t - 1, :]))
            s = torch.cat((vars_[t - 1], act_var))
            mv = [nominal_step(gp.Ky_inv[a], gp.lambdas[a], u, s, gp.X, resid[:, a], gp.sigma_f[a], W[a], b[a])[:2] for a in range(gp.ds)]
            means.append(torch.stack([m for m, _ in mv]))
            vars_.append(torch.stack([v for _, v in mv]))
        return means, [torch.diag(v) for v in vars_]
    if fullcov:
        return O.forward_propagate_fullcov(gp, horizon, x0, Ut, "o2")
    return O.forward_propagate(gp, horizon, x0, Ut, "o2")


def state_term(mean, cov, x_ref, Qw, gamma):
    """One step of the state loop of oracle.cost (src/mpc.py:182-185) / oracle.cost_risk_neutral under the weight ``Qw``."""
    e = mean - x_ref
    if gamma == 0:
        return torch.trace(Qw @ cov) + e @ Qw @ e
    ds = Qw.shape[0]
    return ((1 / gamma) * torch.log(torch.linalg.det(torch.eye(ds, dtype=F64) + gamma * Qw @ cov))
            + e @ torch.linalg.inv(torch.linalg.inv(Qw) + gamma * cov) @ e)


def tracking_cost(means, U, covs, X_ref, U_ref, Q, R, gamma, Q_terminal=None, R_delta=None, last_u=None, terms=None):
    """oracle.cost with x_ref[i], u_ref[j] and the weight of the step.  X_ref (>= H+1, ds), U_ref (>= H, da) or None = zeros: the
    leading rows are used, the terminal weight sits at the call's own step H.  terms: a list that receives the H + 1 state terms."""
    Q, R, X_ref = _t(Q), _t(R), _t(X_ref)
    H = U.shape[0]
    U_ref = torch.zeros((H, U.shape[1]), dtype=F64) if U_ref is None else _t(U_ref)
    Qf = Q if Q_terminal is None else _t(Q_terminal)
    total = 0
    for i in range(H + 1):
        term = state_term(means[i], covs[i], X_ref[i], Qf if i == H else Q, gamma)
        if terms is not None:
            terms.append(float(term.item()))
        total = total + term
    for j in range(H):
        d = U[j, :] - U_ref[j]
        total = total + d @ R @ d
    if R_delta is not None:
        Rd = _t(R_delta)
        dU = torch.diff(torch.cat((_t(last_u).reshape(1, -1), U), dim=0), dim=0)
        for j in range(H):
            total = total + dU[j, :] @ Rd @ dU[j, :]
    return total


def tracking_objective(gp, horizon, x0, U, X_ref, U_ref, Q, R, gamma, Q_terminal=None, R_delta=None, last_u=None, fullcov=False,
                       nominal=None, want_grad=True):
    """dict(cost, grad (H, da), means (H+1, ds), covs (H+1, ds, ds), terms [H+1]) as numpy / float."""
    Ut = _t(U).clone().reshape(horizon, -1).requires_grad_(want_grad)
    means, covs = propagate(gp, horizon, x0, Ut, fullcov, nominal)
    terms = []
    c = tracking_cost(means, Ut, covs, X_ref, U_ref, Q, R, gamma, Q_terminal, R_delta, last_u, terms)
    out = {"cost": float(c.item()), "terms": terms, "means": torch.stack([m.detach() for m in means]).numpy(),
           "covs": torch.stack([s.detach() for s in covs]).numpy()}
    if want_grad:
        c.backward()
        out["grad"] = Ut.grad.detach().numpy().copy()
    return out


def tracking_objectives(gp, horizon, x0, U, R, variants, fullcov=False, nominal=None):
    """Several costs of ONE propagated trajectory (the rollout is the expensive part and depends on none of the cost parameters):
    variants is a list of dicts with the keyword arguments of tracking_cost after (means, U, covs) besides R -- X_ref, U_ref, Q, gamma,
    Q_terminal, R_delta, last_u.  Returns one dict(cost, grad) per variant."""
    Ut = _t(U).clone().reshape(horizon, -1).requires_grad_(True)
    means, covs = propagate(gp, horizon, x0, Ut, fullcov, nominal)
    out = []
    for v in variants:
        c = tracking_cost(means, Ut, covs, v["X_ref"], v.get("U_ref"), v["Q"], R, v["gamma"], v.get("Q_terminal"), v.get("R_delta"),
                          v.get("last_u"))
        (g,) = torch.autograd.grad(c, Ut, retain_graph=True)
        out.append({"cost": float(c.item()), "grad": g.detach().numpy().copy()})
    return out, torch.stack([m.detach() for m in means]).numpy(), torch.stack([s.detach() for s in covs]).numpy()


def general_weight(ds, seed, scale=0.1):
    """A terminal weight that is neither symmetric nor diagonal (the kernels keep Q general), diagonally dominant: invertible, and
    1 + gamma Q_f var > 0 for gamma = -1 at the variances of the synthetic problems."""
    rng = np.random.default_rng(seed)
    return scale * (2.0 * np.eye(ds) + 0.3 * rng.uniform(-1, 1, size=(ds, ds)))


def offset_references(means, U, seed, offset=1.0):
    """References an O(1) distance from a plan's means and inputs (so the cost is O(1) and a relative tolerance means something):
    X_ref (H+1, ds), U_ref (H, da), every row different."""
    rng = np.random.default_rng(seed)
    means, U = np.asarray(means), np.asarray(U)
    return (means + offset * rng.uniform(0.5, 1.0, size=means.shape) * rng.choice([-1.0, 1.0], size=means.shape),
            U + offset * rng.uniform(0.5, 1.0, size=U.shape) * rng.choice([-1.0, 1.0], size=U.shape))
