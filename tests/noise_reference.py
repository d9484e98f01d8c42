"""Float64 CPU reference of the rollout under a noise model (init_cov, action_var, process_var), for tests/test_host_noise.py and
tests/test_gpu_noise.py.  A plain helper module: no fixtures, no collection hooks.

The loops of ``oracle.forward_propagate`` and ``oracle.forward_propagate_fullcov`` restated over the oracle's own single-step functions
(``mean_prop``, ``variance_prop(mode="o2")``, ``covariance_prop(bug_compatible=False)``) with the three parts where the oracle has its
constants:

    S_t     = blkdiag(Sigma_{t-1}, diag(action_var))
    Sigma_0 = diag(diag(init_cov))     diagonal rollout             |  init_cov     full-covariance rollout
    Sigma_t = Sigma^f_t + diag(process_var)                          (t >= 1)

Cost by ``oracle.cost`` / ``oracle.cost_risk_neutral``, gradient by ``backward()`` through the whole loop.  None of the kernels' closed forms
appears here.  At the defaults every operation is the oracle's, in its order: the results are equal, not close (tests/test_host_noise.py).
"""
import numpy as np
import torch

from oracle import gpmpc_oracle as O

F64 = torch.float64


def _t(a):
    return a.to(F64) if isinstance(a, torch.Tensor) else torch.as_tensor(np.array(a, dtype=np.float64))


def defaults(ds, da):
    """(init_cov, action_var, process_var) the library starts with: the oracle's constants and no process noise."""
    return O.INIT_STATE_VAR * np.eye(ds), np.full(da, O.ACTION_NOISE_VAR), np.zeros(ds)


def ladder_noise(ds, da):
    """The model of tests/test_gpu_noise.py for a ladder dimension: a full init_cov, one exactly known input, a process variance per state."""
    rng = np.random.default_rng(5 + ds)
    A = rng.uniform(-1.0, 1.0, (ds, ds))
    init_cov = 0.02 * A @ A.T / ds + np.diag(rng.uniform(1e-4, 3e-2, ds))
    action_var = rng.uniform(1e-4, 1e-2, da)
    action_var[0] = 0.0
    process_var = rng.uniform(1e-5, 2e-3, ds)
    return 0.5 * (init_cov + init_cov.T), action_var, process_var


def _parts(gp, init_cov, action_var, process_var):
    d = defaults(gp.ds, gp.da)
    P = _t(d[0] if init_cov is None else init_cov)
    if P.dim() == 1:
        P = torch.diag(P)
    return P.reshape(gp.ds, gp.ds), _t(d[1] if action_var is None else action_var).reshape(gp.da), _t(d[2] if process_var is None else process_var).reshape(gp.ds)


def _input_cov(gp, cov_prev, action_var):
    S = torch.zeros((gp.D, gp.D), dtype=F64)
    S[:gp.ds, :gp.ds] = cov_prev
    return S + torch.diag(torch.cat((torch.zeros(gp.ds, dtype=F64), action_var)))


def forward_propagate(gp, horizon, x0, U, init_cov=None, action_var=None, process_var=None):
    """``oracle.forward_propagate(mode="o2")`` under the model: lists of H + 1 means (ds,) and DIAGONAL covariance matrices (ds, ds)."""
    P, av, w = _parts(gp, init_cov, action_var, process_var)
    means = [_t(x0).reshape(-1)]
    covs = [torch.diag(torch.diag(P))]
    for t in range(1, horizon + 1):
        u = torch.cat((means[t - 1], U[t - 1, :]))
        S = _input_cov(gp, covs[t - 1], av)
        mu_t, var_t = [], []
        for a in range(gp.ds):
            m, beta, _ = O.mean_prop(gp.Ky_inv[a], gp.lambdas[a], u, S, gp.X, gp.Y[:, a], gp.sigma_f[a])
            v = O.variance_prop(gp.Ky_inv[a], gp.lambdas[a], u, S, gp.X, m, beta, gp.sigma_f[a], "o2")
            mu_t.append(m)
            var_t.append(v)
        means.append(torch.stack(mu_t))
        covs.append(torch.diag(torch.stack(var_t) + w))
    return means, covs


def forward_propagate_fullcov(gp, horizon, x0, U, init_cov=None, action_var=None, process_var=None):
    """``oracle.forward_propagate_fullcov`` under the model: the whole init_cov, process_var on the diagonal of every later covariance."""
    P, av, w = _parts(gp, init_cov, action_var, process_var)
    means = [_t(x0).reshape(-1)]
    covs = [P]
    for t in range(1, horizon + 1):
        u = torch.cat((means[t - 1], U[t - 1, :]))
        S = _input_cov(gp, covs[t - 1], av)
        mu_t, beta_t = [], []
        rows = [[None] * gp.ds for _ in range(gp.ds)]
        for a in range(gp.ds):
            m, beta, _ = O.mean_prop(gp.Ky_inv[a], gp.lambdas[a], u, S, gp.X, gp.Y[:, a], gp.sigma_f[a])
            rows[a][a] = O.variance_prop(gp.Ky_inv[a], gp.lambdas[a], u, S, gp.X, m, beta, gp.sigma_f[a], "o2")
            mu_t.append(m)
            beta_t.append(beta)
        for a in range(gp.ds):
            for b in range(a + 1, gp.ds):
                c = O.covariance_prop(gp.lambdas[a], gp.lambdas[b], u, S, gp.X, mu_t[a], mu_t[b], beta_t[a], beta_t[b],
                                      gp.sigma_f[a], gp.sigma_f[b], bug_compatible=False)
                rows[a][b] = c
                rows[b][a] = c
        means.append(torch.stack(mu_t))
        covs.append(torch.stack([torch.stack(r) for r in rows]) + torch.diag(w))
    return means, covs


def rollout(gp, horizon, x0, U, x_ref, u_ref, Q, R, gamma, init_cov=None, action_var=None, process_var=None, fullcov=False, want_grad=True):
    """dict(cost, means (H+1, ds), vars (H+1, ds) | covs (H+1, ds, ds)[, grad (H, da)]) as numpy: ``oracle.objective_and_gradient`` /
    ``objective_and_gradient_fullcov`` over the loops above."""
    Ut = _t(U).clone().reshape(horizon, -1).requires_grad_(want_grad)
    fp = forward_propagate_fullcov if fullcov else forward_propagate
    means, covs = fp(gp, horizon, x0, Ut, init_cov, action_var, process_var)
    if gamma == 0:
        c = O.cost_risk_neutral(means, Ut, covs, _t(x_ref), _t(u_ref), Q, R)
    else:
        c = O.cost(means, Ut, covs, _t(x_ref), _t(u_ref), Q, R, gamma)
    out = {"cost": float(c.item()), "means": torch.stack([m.detach() for m in means]).numpy()}
    cs = torch.stack([s.detach() for s in covs]).numpy()
    if fullcov:
        out["covs"] = cs
    else:
        out["vars"] = np.stack([np.diag(s) for s in cs])
    if want_grad:
        c.backward()
        out["grad"] = Ut.grad.detach().numpy().copy()
    return out


def nominal_rollout(gp, W, b, horizon, x0, U, x_ref, u_ref, Q, R, gamma, init_cov=None, action_var=None, process_var=None):
    """The diagonal loop above with a linear nominal model m_a(z) = W[a] . z + b[a] (``gp`` holds the RAW targets): each step by
    tests/nominal_reference.py::nominal_step on s = (vars_{t-1}, action_var), process_var added to its variance.  Same dict as ``rollout``."""
    from nominal_reference import nominal_step
    P, av, w = _parts(gp, init_cov, action_var, process_var)
    Wt, bt = _t(W), _t(b).reshape(-1)
    resid = gp.Y - gp.X @ Wt.T - bt
    Ut = _t(U).clone().reshape(horizon, -1).requires_grad_(True)
    means, vars_ = [_t(x0).reshape(-1)], [torch.diag(P).clone()]
    for t in range(1, horizon + 1):
        u = torch.cat((means[t - 1], Ut[t - 1, :]))
        s = torch.cat((vars_[t - 1], av))
        mv = [nominal_step(gp.Ky_inv[a], gp.lambdas[a], u, s, gp.X, resid[:, a], gp.sigma_f[a], Wt[a], bt[a])[:2] for a in range(gp.ds)]
        means.append(torch.stack([m for m, _ in mv]))
        vars_.append(torch.stack([v for _, v in mv]) + w)
    covs = [torch.diag(v) for v in vars_]
    c = O.cost_risk_neutral(means, Ut, covs, _t(x_ref), _t(u_ref), Q, R) if gamma == 0 else O.cost(means, Ut, covs, _t(x_ref), _t(u_ref), Q, R, gamma)
    c.backward()
    return {"cost": float(c.item()), "means": torch.stack([m.detach() for m in means]).numpy(),
            "vars": torch.stack([v.detach() for v in vars_]).numpy(), "grad": Ut.grad.detach().numpy().copy()}


def trajectory(gp, horizon, x0, Ut, init_cov=None, action_var=None, process_var=None):
    """Lists of H + 1 mean and variance tensors attached to the graph of ``Ut`` (for tests/constraints_reference.py::g_of_trajectory)."""
    means, covs = forward_propagate(gp, horizon, x0, Ut, init_cov, action_var, process_var)
    return means, [torch.diagonal(c) for c in covs]
