"""Linear nominal models: the GPs of a :class:`Dynamics` learn what the nominal model leaves over.

The reference accepts nominal models in ``Dynamics`` / ``GaussianProcessRegression`` (src/dynamics.py:27-31, src/gpr.py:24-36) but its
rollout ignores them (src/dynamics.py:64, "TODO: nominal models aren't taken into account here").  For a model that is LINEAR in the
GP input z = (x, u) exact moment matching stays in closed form -- mean ``mu_g + n . u + c``, variance ``v_g + n^T S n + 2 n^T S dmu_g/du``
-- and that is what the HIP rollout propagates when every nominal model of a ``Dynamics`` is a :class:`LinearNominalModel`.
"""
import numpy as np
import torch


class LinearNominalModel(object):
    """m(z) = weights . z + bias for z = (state, action) of dimension D.

    Callable like the reference's ``nominal_model``: a tensor (n, D) -> (n, 1) on the same device, so it serves
    ``GaussianProcessRegression`` (beta, prediction, hyper-parameter training) unchanged.  Immutable: replace the object to change
    the model (``Dynamics`` keys its device pack on the coefficients)."""

    def __init__(self, weights, bias=0.0):
        w = np.array(weights, dtype=np.float64).reshape(-1)
        if w.size < 1 or not np.all(np.isfinite(w)) or not np.isfinite(float(bias)):
            raise ValueError("weights and bias of a LinearNominalModel must be finite, weights non-empty")
        w.setflags(write=False)
        self.weights = w
        self.bias = float(bias)
        self.key = (w.tobytes(), self.bias)
        self._dev = {}

    @classmethod
    def identity(cls, state_dim, action_dim):
        """The ``state_dim`` models of "learn the state difference": GP a corrects m_a(x, u) = x_a."""
        D = int(state_dim) + int(action_dim)
        return [cls(np.eye(D)[a]) for a in range(int(state_dim))]

    def __call__(self, X):
        X = torch.as_tensor(X)
        if X.dim() == 1:
            X = X.reshape(1, -1)
        if X.shape[1] != self.weights.size:
            raise ValueError("LinearNominalModel of dimension %d called with inputs of dimension %d" % (self.weights.size, X.shape[1]))
        k = (X.device, X.dtype)
        w = self._dev.get(k)
        if w is None:
            w = self._dev[k] = torch.as_tensor(self.weights.copy(), device=X.device).to(X.dtype)
        return (X @ w).reshape(-1, 1) + self.bias

    def __repr__(self):
        return "LinearNominalModel(weights=%r, bias=%r)" % (self.weights.tolist(), self.bias)


def stack_linear(models, state_dim, action_dim):
    """(W (ds, D), b (ds,)) of a list of ``state_dim`` LinearNominalModel, or None if the list is not one (None, other callables)."""
    if models is None or len(models) != state_dim or not all(isinstance(m, LinearNominalModel) for m in models):
        return None
    D = state_dim + action_dim
    for m in models:
        if m.weights.size != D:
            raise ValueError("LinearNominalModel of dimension %d in a Dynamics with state_dim + action_dim = %d" % (m.weights.size, D))
    return np.stack([m.weights for m in models]), np.array([m.bias for m in models], dtype=np.float64)
