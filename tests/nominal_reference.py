"""Float64 CPU reference of the rollout with a LINEAR nominal model, for tests/test_host_nominal.py and tests/test_gpu_nominal.py.

Built on the pinned oracle (oracle/gpmpc_oracle.py) and on autograd only -- none of the closed forms of the HIP kernels appear here:

* the GP part of a step is ``oracle.mean_prop`` / ``oracle.variance_prop(mode="o2")`` on the RESIDUAL targets r = y - X n - c;
* the linear part adds ``n . u + c`` to the mean and ``n^T S n`` to the variance;
* the cross term ``2 Cov[n . z, g(z)] = 2 n^T S E[grad g] = 2 n^T S d mu_g / du`` (Stein's lemma) takes d mu_g / du from
  ``torch.autograd.grad(..., create_graph=True)``;
* the cost is ``oracle.cost`` / ``oracle.cost_risk_neutral`` and the gradient ``backward()``.

``quadrature_moments`` is the independent check of the moment formulas themselves: Gauss-Hermite quadrature of the GP posterior
plus the linear model over a 2-D Gaussian input.
"""
import numpy as np
import torch

from oracle import gpmpc_oracle as O

F64 = torch.float64


def _t(a):
    return a.to(F64) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))


def synth_nominal(ds, da, state_weight=1.0, action_weight=0.05, bias=0.01):
    """The nominal model of the tests: identity on the states, ``action_weight`` on every action, one bias.  (W (ds, D), b (ds,))"""
    W = np.zeros((ds, ds + da))
    W[:, :ds] = state_weight * np.eye(ds)
    W[:, ds:] = action_weight
    return W, np.full(ds, bias)


def nominal_step(Ky_inv, lambdas, u, s_diag, X, resid, sigma_f, n, c):
    """Moments of m(z) + g(z), z ~ N(u, diag(s_diag)), for ONE GP trained on ``resid`` and m(z) = n . z + c.
    Tensors are torch float64 (``n``, ``c`` may be numpy / float); ``u`` may carry a graph.  Returns (mean, var, mu_g, var_g)."""
    n, c = _t(n), _t(c)                      # (Python floats welcome: torch.as_tensor(0.01) would be float32)
    if not u.requires_grad:
        u = u.clone().requires_grad_(True)
    S = torch.diag(s_diag)
    mu_g, beta, _ = O.mean_prop(Ky_inv, lambdas, u, S, X, resid, sigma_f)
    var_g = O.variance_prop(Ky_inv, lambdas, u, S, X, mu_g, beta, sigma_f, mode="o2")
    (dmu_du,) = torch.autograd.grad(mu_g, u, create_graph=True)
    mean = mu_g + torch.dot(n, u) + c
    var = var_g + torch.sum(n * n * s_diag) + 2.0 * torch.dot(n * s_diag, dmu_du)
    return mean, var, mu_g, var_g


def nominal_rollout(gp, W, b, horizon, x0, U, x_ref, u_ref, Q, R, gamma, want_grad=True, want_x0_grad=False):
    """Shooting rollout of ``oracle.forward_propagate`` (diagonal covariances, src/dynamics.py:126-191) with the linear nominal model
    m_a(z) = W[a] . z + b[a]; ``gp`` is an ``oracle.GPBundle`` holding the RAW targets.
    Returns dict(cost, grad (H, da), means (H+1, ds), vars (H+1, ds)[, grad_x0 (ds,)]) as numpy / float."""
    W, b = _t(W), _t(b).reshape(-1)
    resid = gp.Y - gp.X @ W.T - b
    Ut = _t(U).clone().reshape(horizon, -1).requires_grad_(want_grad)
    x0t = _t(x0).clone().reshape(-1).requires_grad_(want_grad and want_x0_grad)
    means = [x0t]
    vars_ = [torch.full((gp.ds,), O.INIT_STATE_VAR, dtype=F64)]
    act_var = torch.full((gp.da,), O.ACTION_NOISE_VAR, dtype=F64)
    for t in range(1, horizon + 1):
        u = torch.cat((means[t - 1], Ut[t - 1, :]))
        s = torch.cat((vars_[t - 1], act_var))
        mu_t, var_t = [], []
        for a in range(gp.ds):
            m, v, _, _ = nominal_step(gp.Ky_inv[a], gp.lambdas[a], u, s, gp.X, resid[:, a], gp.sigma_f[a], W[a], b[a])
            mu_t.append(m)
            var_t.append(v)
        means.append(torch.stack(mu_t))
        vars_.append(torch.stack(var_t))
    covs = [torch.diag(v) for v in vars_]
    if gamma == 0:
        c = O.cost_risk_neutral(means, Ut, covs, _t(x_ref), _t(u_ref), Q, R)
    else:
        c = O.cost(means, Ut, covs, _t(x_ref), _t(u_ref), Q, R, gamma)
    out = {"cost": float(c.item()), "means": torch.stack([m.detach() for m in means]).numpy(),
           "vars": torch.stack([v.detach() for v in vars_]).numpy()}
    if want_grad:
        c.backward()
        out["grad"] = Ut.grad.detach().numpy().copy()
        if want_x0_grad:
            out["grad_x0"] = x0t.grad.detach().numpy().copy()
    return out


def assert_reference_is_sane(ref, Q, gamma):
    """For inputs other than the prototyped ones: the reference itself must stay in the regime where the cost is defined."""
    assert np.all(np.isfinite(ref["means"])) and np.all(ref["vars"] > 0), ref["vars"].min()
    assert np.isfinite(ref["cost"])
    assert np.all(1.0 + gamma * np.diag(np.asarray(Q))[None, :] * ref["vars"] > 0)


def quadrature_moments(X, resid, Ky_inv, lambdas, sigma_f, u, s_diag, n, c, order=60):
    """Mean and variance of m(z) + f(z) for z ~ N(u, diag(s)) in TWO input dimensions by order x order Gauss-Hermite quadrature, f the GP
    posterior (mean k(z, X) Ky_inv r, latent variance sf^2 - k Ky_inv k^T): Var = E_z[var_f] + Var_z[m + mean_f].  numpy, float64."""
    X, resid, Ky_inv = np.asarray(X), np.asarray(resid), np.asarray(Ky_inv)
    lambdas, u, s_diag, n = (np.asarray(v, dtype=np.float64) for v in (lambdas, u, s_diag, n))
    assert X.shape[1] == 2
    xs, ws = np.polynomial.hermite.hermgauss(order)
    z0 = u[0] + np.sqrt(2.0 * s_diag[0]) * xs
    z1 = u[1] + np.sqrt(2.0 * s_diag[1]) * xs
    Z = np.stack(np.meshgrid(z0, z1, indexing="ij"), axis=-1).reshape(-1, 2)
    w = np.outer(ws, ws).reshape(-1) / np.pi
    d = Z[:, None, :] - X[None, :, :]
    K = sigma_f ** 2 * np.exp(-0.5 * np.sum(d * d / lambdas, axis=2))
    mean_f = K @ (Ky_inv @ resid)
    var_f = sigma_f ** 2 - np.einsum("ij,jk,ik->i", K, Ky_inv, K)
    tot = Z @ n + c + mean_f
    mean = np.sum(w * tot)
    var = np.sum(w * var_f) + np.sum(w * (tot - mean) ** 2)
    return mean, var
