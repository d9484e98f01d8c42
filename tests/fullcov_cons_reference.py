"""Float64 CPU reference of the chance constraints under the FULL covariance, for tests/test_host_fullcov_cons.py and
tests/test_gpu_fullcov_cons.py.

Built on the pinned oracle (oracle/gpmpc_oracle.py) and on autograd only -- none of the closed forms of the HIP path (the packed step
Jacobian, forward sensitivities, kappa / (2 sd)) appear in the reference:

* the trajectory is ``oracle.forward_propagate_fullcov(gp, H, x0, U, "o2")`` with ``U.requires_grad_()`` (under a noise model: the same loop
  of tests/noise_reference.py, ``forward_propagate_fullcov``);
* ``g[t-1, r] = a_r . mu_t + kappa_r sqrt(a_r^T Sigma_t a_r) - b_r`` straight from the definition, t = 1..H;
* the Jacobian row by row with ``torch.autograd.grad`` (one backward pass per row, run in batches of rows): row (t-1) m_c + r, column tau da + j.

Beside the reference: the tolerance of g (the project's covariance tolerance pushed through the definition) and a numpy restatement of the
packing rule of k_fc_pack_jac, which the host test holds to a dense chain-rule product.
"""
import numpy as np
import torch

from oracle import gpmpc_oracle as O

F64 = torch.float64


def _t(a):
    return a.to(F64) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))


def g_of_full_trajectory(means, covs, A, b, kappa):
    """(H, m_c) tensor of constraint values from lists / stacks of means (ds,) and covariances (ds, ds) (H + 1 entries), by the definition."""
    A, b, kappa = _t(A).reshape(-1, means[0].shape[0]), _t(b).reshape(-1), _t(kappa).reshape(-1)
    rows = []
    for t in range(1, len(means)):
        q = torch.einsum("rk,kl,rl->r", A, covs[t], A)
        rows.append(A @ means[t] + kappa * torch.sqrt(q) - b)
    return torch.stack(rows)


def reference_fullcov_constraints(gp, H, x0, U, A, b, kappa, want_jac=True, noise=None, batched=True, only_rows=None):
    """dict(g (H, m_c), q, sd (H, m_c), g_diag (H, m_c): the DIAGONAL rule on the same trajectory, means (H+1, ds), covs (H+1, ds, ds)
    [, jac (H m_c, H da)]) as numpy.  noise: dict(init_cov, action_var, process_var) of tests/noise_reference.py, or None.
    batched=False: the Jacobian by one ``torch.autograd.grad`` call per row, as tests/constraints_reference.py does it; the default runs the
    same row-wise backward passes in batches of rows (a quarter of the time on c2; tests/test_host_fullcov_cons.py holds the two together on
    every case).  only_rows (with batched=False): the loop over these rows alone, ``jac`` (len(only_rows), H da)."""
    Ut = _t(U).clone().reshape(H, -1).requires_grad_(want_jac)
    if noise is None:
        means, covs = O.forward_propagate_fullcov(gp, H, _t(x0).reshape(-1), Ut, "o2")
    else:
        import noise_reference as NR
        means, covs = NR.forward_propagate_fullcov(gp, H, x0, Ut, **noise)
    g = g_of_full_trajectory(means, covs, A, b, kappa)
    An, bn, kn = np.asarray(A, dtype=np.float64).reshape(-1, gp.ds), np.asarray(b, dtype=np.float64).reshape(-1), np.asarray(kappa, dtype=np.float64).reshape(-1)
    out = {"g": g.detach().numpy().copy(),
           "means": torch.stack([m.detach() for m in means]).numpy(),
           "covs": torch.stack([c.detach() for c in covs]).numpy()}
    out["q"] = np.einsum("rk,tkl,rl->tr", An, out["covs"][1:], An)
    out["sd"] = np.sqrt(out["q"])
    var = np.diagonal(out["covs"][1:], axis1=1, axis2=2)
    out["g_diag"] = out["means"][1:] @ An.T + kn[None, :] * np.sqrt(var @ (An * An).T) - bn[None, :]
    if want_jac:
        m_c = g.shape[1]
        if batched:
            # several rows' backward passes at once: one-hot grad_outputs, the rows as the batch (the passes themselves are those of the
            # loop).  A chunk holds as many rows as keep its N x N intermediates within ~16 MB: beyond that the batch is slower than the loop.
            R, eye = H * m_c, torch.eye(H * m_c, dtype=F64)
            chunk = max(1, min(R, int(2e6 // (gp.X.shape[0] ** 2))))
            parts = [torch.autograd.grad(g.reshape(-1), Ut, grad_outputs=eye[i:i + chunk], is_grads_batched=True, retain_graph=True)[0]
                     for i in range(0, R, chunk)]
            jac = torch.cat(parts).reshape(R, -1).numpy().copy()
        else:
            which = list(range(H * m_c)) if only_rows is None else list(only_rows)
            jac = np.zeros((len(which), Ut.numel()))
            for k, i in enumerate(which):
                (row,) = torch.autograd.grad(g[i // m_c, i % m_c], Ut, retain_graph=True)
                jac[k] = row.reshape(-1).numpy()
        out["jac"] = jac
    return out


def g_tolerance(ref, A, kappa):
    """(H, m_c): 1e-5 sum_k |a_k mu_k| + kappa dq / (2 sd_ref) + 1e-9 with dq = sum_kl |a_k a_l| (1e-4 |Sigma_kl| + 1e-6 max |Sigma_t|): the
    project's covariance tolerance (tests/test_gpu_parity.py: rtol 1e-4, atol 1e-6 of the largest entry) pushed through the definition of g,
    d sd = d q / (2 sd)."""
    A, kappa = np.asarray(A, dtype=np.float64), np.asarray(kappa, dtype=np.float64).reshape(-1)
    mu, S = ref["means"][1:], ref["covs"][1:]
    aa = np.abs(A[:, :, None] * A[:, None, :])                                       # (m_c, ds, ds)
    dS = 1e-4 * np.abs(S) + 1e-6 * np.abs(S).max(axis=(1, 2))[:, None, None]         # (H, ds, ds)
    dq = np.einsum("rkl,tkl->tr", aa, dS)
    return 1e-5 * np.abs(mu[:, None, :] * A[None, :, :]).sum(axis=2) + kappa[None, :] * dq / (2.0 * ref["sd"]) + 1e-9


# ---------------------------------------------------------------------------------------------------------------------------------
# the packing rule of k_fc_pack_jac (csrc/fullcov_cons.hip), restated
# ---------------------------------------------------------------------------------------------------------------------------------
def tri_pairs(ds):
    """The (k, l), k <= l, of the row-major upper triangle."""
    return [(k, l) for k in range(ds) for l in range(k, ds)]


def pack_jacobian(dmean_du, dmean_dS, dcov_du, dcov_dS, ds, da):
    """One step: dmean_du (ds, D), dmean_dS (ds, D, D), dcov_du (ds, ds, D), dcov_dS (ds, ds, D, D) -> (p, p + da), p = ds + ds (ds + 1) / 2.
    Rows (mu'_a, Sigma'_ab for a <= b), columns (mu_k, Sigma_kl for k <= l, u_j).  Sigma_kl = Sigma_lk is ONE variable: its column is
    d/dS_kl + d/dS_lk; the diagonal's is d/dS_kk.  Only the state block of dS is read."""
    tri = tri_pairs(ds)
    p = ds + len(tri)
    J = np.zeros((p, p + da))
    rows = [(dmean_du[a], dmean_dS[a]) for a in range(ds)] + [(dcov_du[a, b], dcov_dS[a, b]) for a, b in tri]
    for r, (du, dS) in enumerate(rows):
        J[r, :ds] = du[:ds]
        for c, (k, l) in enumerate(tri):
            J[r, ds + c] = dS[k, k] if k == l else dS[k, l] + dS[l, k]
        J[r, p:] = du[ds:]
    return J
