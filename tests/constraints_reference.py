"""Float64 CPU reference of the state chance constraints, for tests/test_host_constraints.py and tests/test_gpu_constraints.py.

Built on the pinned oracle (oracle/gpmpc_oracle.py) and on autograd only -- none of the closed forms of the HIP kernel (forward
sensitivities, kappa / (2 sd)) appear here:

* the trajectory is ``oracle.forward_propagate(gp, H, x0, U, "o2")`` with ``U.requires_grad_()`` (with a linear nominal model: the step of
  tests/nominal_reference.py, ``nominal_step``, in the same loop as its ``nominal_rollout``);
* ``g[t-1, r] = a_r . mu_t + kappa_r sqrt(sum_k a_rk^2 var_tk) - b_r`` straight from the definition, t = 1..H;
* the Jacobian row by row with ``torch.autograd.grad``: row (t-1) m_c + r, column tau da + j.
"""
import numpy as np
import torch

from oracle import gpmpc_oracle as O

F64 = torch.float64


def _t(a):
    return a.to(F64) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))


def _trajectory(gp, H, x0, Ut, nominal=None):
    """Lists of H + 1 mean tensors (ds,) and variance tensors (ds,), attached to the graph of ``Ut``."""
    if nominal is None:
        means, covs = O.forward_propagate(gp, H, _t(x0).reshape(-1), Ut, "o2")
        return means, [torch.diagonal(c) for c in covs]
    from nominal_reference import nominal_step
    W, b = _t(nominal[0]), _t(nominal[1]).reshape(-1)
    resid = gp.Y - gp.X @ W.T - b
    means = [_t(x0).reshape(-1)]
    vars_ = [torch.full((gp.ds,), O.INIT_STATE_VAR, dtype=F64)]
    act_var = torch.full((gp.da,), O.ACTION_NOISE_VAR, dtype=F64)
    for t in range(1, H + 1):
        u = torch.cat((means[t - 1], Ut[t - 1, :]))
        s = torch.cat((vars_[t - 1], act_var))
        mv = [nominal_step(gp.Ky_inv[a], gp.lambdas[a], u, s, gp.X, resid[:, a], gp.sigma_f[a], W[a], b[a])[:2] for a in range(gp.ds)]
        means.append(torch.stack([m for m, _ in mv]))
        vars_.append(torch.stack([v for _, v in mv]))
    return means, vars_


def g_of_trajectory(means, vars_, A, b, kappa):
    """(H, m_c) tensor of constraint values from lists / stacks of means and variances (H + 1 entries), by the definition."""
    A, b, kappa = _t(A).reshape(-1, means[0].shape[0]), _t(b).reshape(-1), _t(kappa).reshape(-1)
    rows = []
    for t in range(1, len(means)):
        q = (A * A) @ vars_[t]
        rows.append(A @ means[t] + kappa * torch.sqrt(q) - b)
    return torch.stack(rows)


def reference_constraints(gp, H, x0, U, A, b, kappa, nominal=None, want_jac=True):
    """dict(g (H, m_c), sd (H, m_c), means (H+1, ds), vars (H+1, ds)[, jac (H m_c, H da)]) as numpy."""
    Ut = _t(U).clone().reshape(H, -1).requires_grad_(want_jac)
    means, vars_ = _trajectory(gp, H, x0, Ut, nominal)
    g = g_of_trajectory(means, vars_, A, b, kappa)
    A_t = _t(A).reshape(-1, gp.ds)
    out = {"g": g.detach().numpy().copy(),
           "means": torch.stack([m.detach() for m in means]).numpy(),
           "vars": torch.stack([v.detach() for v in vars_]).numpy()}
    out["sd"] = np.sqrt(np.stack([(A_t.numpy() ** 2) @ v for v in out["vars"][1:]]))
    if want_jac:
        m_c = g.shape[1]
        jac = np.zeros((H * m_c, Ut.numel()))
        for t in range(H):
            for r in range(m_c):
                (row,) = torch.autograd.grad(g[t, r], Ut, retain_graph=True)
                jac[t * m_c + r] = row.reshape(-1).numpy()
        out["jac"] = jac
    return out


def reference_cost(gp, H, x0, U, x_ref, u_ref, Q, R, gamma):
    """Cost of a plan by the pinned oracle (mode "o2", no gradient)."""
    return O.objective_and_gradient(gp, H, x0, U, x_ref, u_ref, Q, R, gamma, mode="o2", want_grad=False)["cost"]
