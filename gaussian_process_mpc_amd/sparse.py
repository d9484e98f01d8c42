"""Sparse GP dynamics: FITC inducing points, built and updated on the device (no reference counterpart).

M pseudo-inputs ``Z`` summarise N >> M observations; the planner's cost then depends on M only.  A FITC posterior has the shape the
rollout kernels consume -- mean ``k_*^T alpha``, variance ``sigma_f^2 - k_*^T Q k_*`` -- so the pack is built from ``(Z, alpha, Q)``
through ``gpmpc_pack_build_beta`` and no rollout kernel knows about it.  What lives here is what produces ``(alpha, Q)``, in the
WHITENED form of include/gpmpc.h ("Sparse GP"; DESIGN.md section 3h says why not the textbook form):

    Kmm = k(Z,Z) + jitter I,  W = chol(Kmm)^-1,  v_n = W k(Z, x_n),  Lambda_n = sigma_f^2 + sigma_n^2 - |v_n|^2
    G = sum_n v_n v_n^T / Lambda_n,  r = sum_n v_n y_n^T / Lambda_n,  Binv = (I + G)^-1,  alpha = W^T Binv r,  Q = W^T (I - Binv) W

Everything that touches N is HIP (csrc/sparse.hip).  torch is plumbing, as ``torch.linalg.inv`` is for the dense GP: the Cholesky
factor of Kmm, its triangular inverse, the inverse of B and the elementwise residual targets of a linear nominal model.

Out of scope: FITC marginal-likelihood training (train the hyper-parameters on a dense subset with ``update_hyperparams`` and set
them here), VFE / DTC variants, moving the inducing points along the previous plan, a different ``Z`` per GP, multi-GPU broadcast of
the update.
"""
import ctypes

import numpy as np
import torch

from ._lib import check, lib, ptr, require_gpu, stream_ptr, host_doubles
from .dynamics import Dynamics
from .nominal import stack_linear
from .rollout import GPPack, _dev


def select_inducing(X, M, lambdas, method="farthest", seed=0, return_index=False):
    """M rows of X (N, D) to serve as inducing points.  "farthest": greedy farthest-point selection in the lambda-metric
    d^2(x, z) = sum_d (x_d - z_d)^2 / lambda_d, O(N M), starting from the row ``seed % N``; "random": a seeded draw without
    replacement.  A selection on the host, not path arithmetic."""
    X = np.asarray(X.detach().cpu() if isinstance(X, torch.Tensor) else X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be (N, D)")
    N, M = X.shape[0], int(M)
    if not 1 <= M <= N:
        raise ValueError("M must lie in 1...N = %d, got %d" % (N, M))
    if method == "random":
        idx = np.sort(np.random.default_rng(seed).choice(N, size=M, replace=False))
    elif method == "farthest":
        lam = np.broadcast_to(np.asarray(lambdas, dtype=np.float64).reshape(-1, X.shape[1])[0], (X.shape[1],))
        Xs = X / np.sqrt(lam)
        idx = np.empty(M, dtype=np.int64)
        idx[0] = int(seed) % N
        d = np.sum((Xs - Xs[idx[0]]) ** 2, axis=1)
        for k in range(1, M):
            idx[k] = int(np.argmax(d))
            d = np.minimum(d, np.sum((Xs - Xs[idx[k]]) ** 2, axis=1))
    else:
        raise ValueError('method must be "farthest" or "random", got %r' % (method,))
    Z = np.ascontiguousarray(X[idx])
    return (Z, idx) if return_index else Z


def _check_inducing(Z, D):
    Z = np.asarray(Z.detach().cpu() if isinstance(Z, torch.Tensor) else Z, dtype=np.float64)
    if Z.ndim != 2 or Z.shape[0] < 1 or Z.shape[1] != D:
        raise ValueError("inducing points must be (M, %d) with M >= 1, got shape %r" % (D, Z.shape))
    if not np.all(np.isfinite(Z)):
        raise ValueError("inducing points must be finite")
    return np.ascontiguousarray(Z)


class SparseGPState(object):
    """One hyper-parameter group: the GPs that share (lambda, sigma_f, sigma_n) share W, G, Binv and Q; their targets are the columns of r.

    ``fit(X, Y)`` builds from scratch, ``add(X, Y)`` accumulates more rows (both O(N M^2) on the device, never an N x M matrix),
    ``append(x, y)`` is the O(M^2) rank-one update of one observation and ``refresh()`` recomputes Binv from G by a fresh inverse and
    then alpha and Q: O(M^3) and NO pass over the data.  Every ``refresh_every`` appends (64, the figure of the dense incremental path)
    a refresh bounds the round-off of the rank-one updates.  ``fit``, ``add`` and ``refresh`` synchronise and raise if min Lambda_n is
    not positive and finite; ``append`` never synchronises.  ``remove(x, y)`` and ``replace(x_old, y_old, x_new, y_new)`` are the
    O(M^2) steps of a fixed-size window (each one rank-one step towards ``refresh_every``); ``rebase(X, Y)`` re-accumulates G and r
    over the rows held, which is what bounds the round-off of a long chain of replacements."""

    def __init__(self, Z, lambdas, sigma_f, sigma_n, jitter=None, chunk=0, device=None, noise_var=None):
        self.device = device if device is not None else require_gpu()
        lam = np.ascontiguousarray(np.asarray(lambdas, dtype=np.float64).reshape(-1))
        self.D = lam.shape[0]
        Zh = _check_inducing(Z, self.D)
        self.M = Zh.shape[0]
        self.lambdas, self.sigma_f, self.sigma_n = lam, float(sigma_f), float(sigma_n)
        # (noise_var: what sits in Lambda beside sigma_f^2; the dense GP class puts float32(sigma_n^2) on its diagonal and passes that here)
        self.noise_var = float(sigma_n) ** 2 if noise_var is None else float(noise_var)
        self.jitter = 1e-6 * self.sigma_f ** 2 if jitter is None else float(jitter)
        if chunk < 0 or chunk % 64:
            raise ValueError("chunk must be 0 (default) or a positive multiple of 64, got %r" % (chunk,))
        self.chunk = int(chunk)
        self.refresh_every = 64
        self._appends = 0
        self.n_targets = None
        self.Z = torch.as_tensor(Zh, device=self.device)
        self._ws = {}
        self._build_w()

    # -- plumbing ----------------------------------------------------------------------------
    def _workspace(self, key, nbytes):
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = self._ws[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
        return ws

    def _build_w(self):
        M = self.M
        Kmm = torch.empty((M, M), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().gpmpc_build_ky(M, self.D, ptr(self.Z), host_doubles(self.lambdas)[1], self.sigma_f, self.jitter, None, ptr(Kmm),
                                       stream_ptr()), "gpmpc_build_ky")
        L = torch.linalg.cholesky(Kmm)
        eye = torch.eye(M, dtype=torch.float64, device=self.device)
        self.W = torch.tril(torch.linalg.solve_triangular(L, eye, upper=False)).contiguous()

    def _alloc(self, n_targets):
        n_targets = int(n_targets)
        if self.n_targets == n_targets:
            return
        M, z = self.M, lambda *s: torch.zeros(s, dtype=torch.float64, device=self.device)  # noqa: E731
        self.n_targets = n_targets
        self.G, self.Q, self.r, self.alpha = z(M, M), z(M, M), z(M, n_targets), z(M, n_targets)
        self.Binv = torch.eye(M, dtype=torch.float64, device=self.device)
        self.stats = torch.tensor([0.0, float("inf")], dtype=torch.float64, device=self.device)
        self._appends = 0

    def _accumulate(self, X, Y, accumulate, keep=False):
        """``keep``: overwrite (``accumulate = 0``) into the tensors the state holds instead of fresh ones."""
        X, Y = _dev(X, self.device).reshape(-1, self.D), _dev(Y, self.device)
        Y = Y.reshape(X.shape[0], -1)
        if accumulate and self.n_targets is None:
            accumulate = 0
        if not accumulate and not keep:
            self.n_targets = None
        if self.n_targets is None:
            self._alloc(Y.shape[1])
        if Y.shape[1] != self.n_targets:
            raise ValueError("Y has %d target columns, the state holds %d" % (Y.shape[1], self.n_targets))
        n = X.shape[0]
        nb = lib().gpmpc_sparse_accumulate_workspace_bytes(n, self.D, self.M, self.n_targets, self.chunk)
        ws = self._workspace("acc", nb)
        with torch.cuda.device(self.device):
            check(lib().gpmpc_sparse_accumulate(n, self.D, self.M, self.n_targets, ptr(X), ptr(Y), Y.shape[1], ptr(self.Z), ptr(self.W), self.M,
                                                host_doubles(self.lambdas)[1], self.sigma_f, self.noise_var, self.chunk, int(bool(accumulate)),
                                                ptr(self.G), ptr(self.r), ptr(self.stats), ctypes.c_void_p(ws.data_ptr()), nb, stream_ptr()),
                  "gpmpc_sparse_accumulate")

    # -- public ------------------------------------------------------------------------------
    def fit(self, X, Y):
        """From scratch on X (N, D), Y (N, n_targets): G, r, then ``refresh``."""
        self._accumulate(X, Y, 0)
        self.refresh()
        return self

    def add(self, X, Y):
        """More rows in bulk (``accumulate = 1``), then ``refresh``."""
        self._accumulate(X, Y, 1)
        self.refresh()
        return self

    def refresh(self, check_lambda=True):
        """Binv from G by a fresh inverse (symmetrised: the kernels read one triangle), then alpha and Q.  O(M^3), no pass over the data."""
        if self.n_targets is None:
            raise RuntimeError("no data: call fit first")
        M = self.M
        if check_lambda:
            ml = self.min_lambda                         # (synchronises)
            if not (np.isfinite(ml) and ml > 0.0):
                raise FloatingPointError("sparse GP: min Lambda_n = %r is not positive and finite (FITC needs sigma_f^2 + sigma_n^2 > |v_n|^2: "
                                         "raise sigma_n or the jitter)" % (ml,))
        B = self.G + torch.eye(M, dtype=torch.float64, device=self.device)
        Bi = torch.linalg.inv(B) if check_lambda else torch.linalg.inv_ex(B, check_errors=False).inverse
        self.Binv.copy_(0.5 * (Bi + Bi.T))
        nb = lib().gpmpc_sparse_finish_workspace_bytes(M, self.n_targets)
        ws = self._workspace("fin", nb)
        with torch.cuda.device(self.device):
            check(lib().gpmpc_sparse_finish(M, self.n_targets, ptr(self.W), M, ptr(self.Binv), ptr(self.r), ptr(self.alpha), ptr(self.Q),
                                            ctypes.c_void_p(ws.data_ptr()), nb, stream_ptr()), "gpmpc_sparse_finish")
        self._appends = 0
        return self

    def append(self, x, y):
        """One observation x (D,), y (n_targets,), rank-one and in place on the device; does not synchronise (the periodic refresh of
        every ``refresh_every`` appends skips its host-side check for the same reason: ``min_lambda`` shows it on demand)."""
        y = _dev(y, self.device).reshape(-1)
        if self.n_targets is None:
            self._alloc(y.shape[0])
        x = _dev(x, self.device).reshape(-1)
        if x.shape[0] != self.D or y.shape[0] != self.n_targets:
            raise ValueError("append takes x (%d,) and y (%d,)" % (self.D, self.n_targets))
        nb = lib().gpmpc_sparse_append_workspace_bytes(self.M, self.n_targets)
        ws = self._workspace("app", nb)
        with torch.cuda.device(self.device):
            check(lib().gpmpc_sparse_append(self.D, self.M, self.n_targets, ptr(x), ptr(y), ptr(self.Z), ptr(self.W), self.M,
                                            host_doubles(self.lambdas)[1], self.sigma_f, self.noise_var, ptr(self.G), ptr(self.r), ptr(self.Binv),
                                            ptr(self.Q), ptr(self.alpha), ptr(self.stats), ctypes.c_void_p(ws.data_ptr()), nb, stream_ptr()),
                  "gpmpc_sparse_append")
        self._stepped()
        return self

    def _stepped(self):
        """One rank-one step (append, remove or replace) towards the periodic refresh."""
        self._appends += 1
        if self.refresh_every and self._appends >= self.refresh_every:
            self.refresh(check_lambda=False)

    def _rank_one(self, name, rows):
        """gpmpc_sparse_remove / _replace on device rows [(x, y), ...]; does not synchronise."""
        if self.n_targets is None:
            raise RuntimeError("no data: call fit first")
        ptrs = []
        for x, y in rows:
            x, y = _dev(x, self.device).reshape(-1), _dev(y, self.device).reshape(-1)
            if x.shape[0] != self.D or y.shape[0] != self.n_targets:
                raise ValueError("%s takes x (%d,) and y (%d,)" % (name, self.D, self.n_targets))
            ptrs += [x, y]
        fn = "gpmpc_sparse_" + name
        nb = getattr(lib(), fn + "_workspace_bytes")(self.M, self.n_targets)
        ws = self._workspace(name[:3], nb)
        with torch.cuda.device(self.device):
            check(getattr(lib(), fn)(self.D, self.M, self.n_targets, *[ptr(t) for t in ptrs], ptr(self.Z), ptr(self.W), self.M,
                                     host_doubles(self.lambdas)[1], self.sigma_f, self.noise_var, ptr(self.G), ptr(self.r), ptr(self.Binv),
                                     ptr(self.Q), ptr(self.alpha), ptr(self.stats), ctypes.c_void_p(ws.data_ptr()), nb, stream_ptr()), fn)
        self._stepped()
        return self

    def remove(self, x, y):
        """Take out one observation the state holds (the inverse of ``append``, O(M^2), in place, no synchronisation).  Afterwards
        ``min_lambda`` is a lower bound on the Lambda of the rows held, not their minimum; ``rebase`` restores it."""
        return self._rank_one("remove", [(x, y)])

    def replace(self, x_old, y_old, x_new, y_new):
        """``remove(x_old, y_old)`` and ``append(x_new, y_new)`` in one pass over G, Binv and Q (the step of a full window); counts as
        ONE rank-one step towards ``refresh_every``.  Does not synchronise."""
        return self._rank_one("replace", [(x_old, y_old), (x_new, y_new)])

    def rebase(self, X, Y):
        """Re-accumulate G, r and the stats over the rows X (N, D), Y (N, n_targets) the state is meant to hold, into the tensors it
        has (no reallocation), then ``refresh(check_lambda=False)``: what a chain of replacements has drifted by is gone (a fresh
        inverse alone does not remove it: the drift sits in G and r).  Bit for bit what ``fit`` gives on the same rows in the same order."""
        if self.n_targets is None:
            raise RuntimeError("no data: call fit first")
        self._accumulate(X, Y, 0, keep=True)
        return self.refresh(check_lambda=False)

    @property
    def num_obs(self):
        return 0 if self.n_targets is None else int(self.stats[0].item())

    @property
    def min_lambda(self):
        return float("inf") if self.n_targets is None else float(self.stats[1].item())

    def predict(self, Xs, covar=True):
        """Posterior at Xs (p, D) through the existing ``gpmpc_predict`` with (Z, alpha, Q): mean (p, n_targets) and, with ``covar``, the
        latent covariance (p, p) = K** - K* Q K*^T shared by the group's GPs.  Device tensors."""
        if self.n_targets is None:
            raise RuntimeError("no data: call fit first")
        Xp = _dev(Xs, self.device).reshape(-1, self.D)
        p, M = Xp.shape[0], self.M
        mean = torch.empty((self.n_targets, p), dtype=torch.float64, device=self.device)
        cov = torch.empty((p, p), dtype=torch.float64, device=self.device) if covar else None
        nb = lib().gpmpc_predict_workspace_bytes(M, self.D, p)
        ws = self._workspace("pred", nb)
        alpha_t = self.alpha.T.contiguous()
        with torch.cuda.device(self.device):
            for a in range(self.n_targets):
                check(lib().gpmpc_predict(M, self.D, ptr(self.Z), host_doubles(self.lambdas)[1], self.sigma_f, ptr(alpha_t[a]), ptr(self.Q), 0.0,
                                          p, ptr(Xp), None, ptr(mean[a]), ptr(cov) if (covar and a == 0) else None,
                                          ctypes.c_void_p(ws.data_ptr()), nb, stream_ptr()), "gpmpc_predict")
        return mean.T.contiguous(), cov


class SparseDynamics(Dynamics):
    """A :class:`Dynamics` whose GPs are FITC sparse GPs on shared inducing points ``inducing`` (M, state_dim + action_dim): a drop-in
    for ``RiskSensitiveMPC`` (``mpc.dynamics = SparseDynamics(...)`` or ``mpc.use_inducing_points(Z)``), ``Simulator`` and every solver.

    ``gpr_err[i]`` hold the hyper-parameters (set_lambdas / set_sigma_f / set_sigma_n) and a truthful ``num_train``; they hold no
    matrices.  GPs with bit-identical hyper-parameters share one :class:`SparseGPState`.  A single observation takes the rank-one path,
    many go through ``add``.  ``pack()`` builds ``GPPack(Z, alpha, Q, y_is_beta=True)`` once and refills it in place after every data
    update: M is constant, so a closed loop keeps one pack handle and one captured callback graph.  Linear nominal models are
    supported (the accumulators see the residual targets, the pack gets the model); other callables are refused.  The observations
    are kept in capacity-doubling device buffers (``keep_data``) so that ``set_inducing`` and hyper-parameter changes can refit; with
    ``keep_data=False`` those raise.  ``max_train`` and ``async_rebuild=True`` raise ``ValueError``.

    ``window`` (an int >= 1; needs ``keep_data``) makes the model forget: the observations live in a ring of exactly ``window`` rows,
    and once it is full a single observation REPLACES the oldest one (``window_slot``) in every hyper-parameter group by the O(M^2)
    rank-one replacement, the old row read from the ring on the device.  A bulk call that would overflow the window keeps the newest
    ``window`` rows in chronological order, refits and resets the slot to 0 (the rule of ``Dynamics._trim_to_window``).  After
    ``rebase_every`` replacements (default ``window``: the amortised cost per step stays O(M^2); 0: never) G and r are re-accumulated
    from the ring, which bounds the round-off of the chain.  M, the pack handle and the captured callback graph
    stay what they were."""

    def __init__(self, state_dim, action_dim, inducing, nominal_models=None, jitter=None, keep_data=True, chunk=0, window=None):
        if nominal_models is not None and stack_linear(nominal_models, state_dim, action_dim) is None:
            raise ValueError("SparseDynamics supports LinearNominalModel nominal models only (one per state dimension)")
        Z = _check_inducing(inducing, state_dim + action_dim)
        if chunk < 0 or chunk % 64:
            raise ValueError("chunk must be 0 (default) or a positive multiple of 64, got %r" % (chunk,))
        if jitter is not None and not (np.isfinite(jitter) and jitter >= 0):
            raise ValueError("jitter must be finite and non-negative, got %r" % (jitter,))
        if window is not None:
            if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1:
                raise ValueError("window must be an int >= 1 or None, got %r" % (window,))
            if not keep_data:
                raise ValueError("window needs the observations it forgets: SparseDynamics(keep_data=True)")
        super().__init__(state_dim, action_dim, nominal_models)       # (argument errors come first: this needs the device)
        self.D = state_dim + action_dim
        self._Z = Z
        self.jitter = jitter
        self.keep_data = bool(keep_data)
        self.chunk = int(chunk)
        self.num_train = 0
        self._Xbuf = self._Ybuf = None                   # capacity-doubling device buffers [cap][D], [cap][ds] (raw targets)
        self._groups = None                              # [(columns, SparseGPState)]
        self._group_key = None
        self._data_version = 0
        self._z_version = 0
        self._row = None                                 # pinned staging row of one observation
        self._window = None if window is None else int(window)
        self.window_slot = 0                             # ring row the next replacement overwrites (the oldest observation)
        self.rebase_every = 0 if window is None else int(window)
        self._replacements = 0                           # since the last accumulation from the ring

    # -- refused settings ----------------------------------------------------------------------
    @property
    def max_train(self):
        return None

    @max_train.setter
    def max_train(self, value):
        if value is not None:
            raise ValueError("max_train (fixed-size window) is not supported by SparseDynamics: the inducing points bound the cost")

    @property
    def window(self):
        return self._window

    @property
    def M(self):
        return self._Z.shape[0]

    @property
    def inducing(self):
        return self._Z.copy()

    def set_inducing(self, Z):
        """Other inducing points (any M): refit from the kept data; the pack is re-created when M changed."""
        Z = _check_inducing(Z, self.D)
        if self.num_train and not self.keep_data:
            raise RuntimeError("set_inducing needs the observations: SparseDynamics(keep_data=True)")
        self._Z = Z
        self._z_version += 1
        self._groups = None

    # -- hyper-parameter groups ------------------------------------------------------------------
    def _hyper_key(self):
        return [(g.log_lambdas, g.log_lambdas._version, g.log_sigma_f, g.log_sigma_f._version, g.log_sigma_n, g.log_sigma_n._version)
                for g in self.gpr_err]

    @staticmethod
    def _same_hyper(a, b):
        return a is not None and b is not None and len(a) == len(b) and all(
            x[0] is y[0] and x[1] == y[1] and x[2] is y[2] and x[3] == y[3] and x[4] is y[4] and x[5] == y[5] for x, y in zip(a, b))

    def _nominal_arrays(self):
        return stack_linear(self.nominal_models, self.state_dim, self.action_dim) if self.nominal_models is not None else None

    def _residual(self, X, Y):
        """Residual targets Y - X W_n^T - b_n of the linear nominal model (elementwise torch), or Y itself."""
        lin = self._nominal_arrays()
        if lin is None:
            return Y
        Wn = torch.as_tensor(lin[0], device=self.device)
        bn = torch.as_tensor(lin[1], device=self.device)
        return Y - X @ Wn.T - bn

    def _ensure_groups(self):
        """The states of the current hyper-parameters / inducing points; (re)fitted from the kept data when either changed."""
        key = self._hyper_key() + [self._nominal_key()]
        if self._groups is not None and self._same_hyper(key[:-1], self._group_key[:-1]) and key[-1] == self._group_key[-1]:
            return self._groups
        if self._groups is not None and self.num_train and not self.keep_data:
            raise RuntimeError("hyper-parameters changed after data was added: SparseDynamics(keep_data=True) is needed to refit")
        if self._groups is None and self.num_train and not self.keep_data:
            raise RuntimeError("set_inducing after data was added needs SparseDynamics(keep_data=True)")
        by = {}
        for a, g in enumerate(self.gpr_err):
            by.setdefault((g.get_lambdas().tobytes(), float(g.get_sigma_f()), float(g._noise_var())), []).append(a)
        groups = []
        for cols in by.values():
            g = self.gpr_err[cols[0]]
            st = SparseGPState(self._Z, g.get_lambdas(), g.get_sigma_f(), g.get_sigma_n(), jitter=self.jitter, chunk=self.chunk,
                               device=self.device, noise_var=g._noise_var())
            groups.append((cols, st))
        self._groups, self._group_key = groups, key
        if self.num_train:
            X, Y = self._rows()
            R = self._residual(X, Y)
            for cols, st in groups:
                st.fit(X, R[:, cols].contiguous())
            self._replacements = 0
        self._data_version += 1
        return groups

    # -- data ------------------------------------------------------------------------------------
    def _rows(self):
        """The observations held, oldest first (views of the buffers; copies when the ring has wrapped)."""
        n, s = self.num_train, self.window_slot
        if s == 0:
            return self._Xbuf[:n], self._Ybuf[:n]
        return torch.cat((self._Xbuf[s:n], self._Xbuf[:s])), torch.cat((self._Ybuf[s:n], self._Ybuf[:s]))

    def _store(self, X, Y):
        n, k = self.num_train, X.shape[0]
        if not self.keep_data:
            self.num_train = n + k
            return
        if self._window is not None and self._Xbuf is None:     # the ring: exactly `window` rows, once
            self._Xbuf = torch.empty((self._window, self.D), dtype=torch.float64, device=self.device)
            self._Ybuf = torch.empty((self._window, self.state_dim), dtype=torch.float64, device=self.device)
        cap = 0 if self._Xbuf is None else self._Xbuf.shape[0]
        if n + k > cap:
            new = max(256, cap)
            while new < n + k:
                new *= 2
            Xb = torch.empty((new, self.D), dtype=torch.float64, device=self.device)
            Yb = torch.empty((new, self.state_dim), dtype=torch.float64, device=self.device)
            if n:
                Xb[:n].copy_(self._Xbuf[:n])
                Yb[:n].copy_(self._Ybuf[:n])
            self._Xbuf, self._Ybuf = Xb, Yb
        self._Xbuf[n:n + k].copy_(X)
        self._Ybuf[n:n + k].copy_(Y)
        self.num_train = n + k

    def append_train_data(self, state, action, next_state, incremental=True, async_rebuild=None, refresh=None):
        """(state, action, next_state) observations, one or many.  One observation: the O(M^2) rank-one update (whatever
        ``incremental`` says: there is no O(N) alternative worth having); many: one bulk accumulation and a refresh.  ``refresh`` is
        accepted for interface compatibility and ignored (the periodic refresh is ``SparseGPState.refresh_every``)."""
        if async_rebuild:
            raise ValueError("async_rebuild=True is not supported by SparseDynamics (there is no O(N^3) rebuild to hide)")
        if refresh is not None and refresh not in ("rebuild", "newton"):
            raise ValueError("refresh must be 'rebuild' or 'newton', got %r" % (refresh,))
        state, action, next_state = np.asarray(state, dtype=np.float64), np.asarray(action, dtype=np.float64), np.asarray(next_state, dtype=np.float64)
        single = state.ndim == 1
        if single:
            x = np.concatenate((state, action.reshape(-1)))[None, :]
            y = next_state.reshape(1, self.state_dim)
        else:
            if action.ndim == 1:
                action = action[:, None]
            x = np.concatenate((state, action), axis=1)
            y = next_state.reshape(-1, self.state_dim)
        if x.shape[1] != self.D or y.shape[0] != x.shape[0]:
            raise ValueError("observations must be (state (%d), action (%d), next_state (%d))" % (self.state_dim, self.action_dim, self.state_dim))
        groups = self._ensure_groups()                   # (before the new rows are stored: a refit must not see them twice)
        xy = torch.as_tensor(np.concatenate((x, y), axis=1), device=self.device)      # one host-to-device copy
        X, Y = xy[:, :self.D].contiguous(), xy[:, self.D:].contiguous()
        if self._window is not None and self.num_train + X.shape[0] > self._window:
            self._window_update(groups, X, Y, single)
            for g in self.gpr_err:
                g.num_train = self.num_train
            self._data_version += 1
            return
        self._store(X, Y)
        R = self._residual(X, Y)
        for cols, st in groups:
            Rg = R[:, cols].contiguous()
            if single and st.n_targets is not None:
                st.append(X[0], Rg[0])
            elif st.n_targets is None:
                st.fit(X, Rg)
            else:
                st.add(X, Rg)
        for g in self.gpr_err:
            g.num_train = self.num_train
        self._data_version += 1

    def _window_update(self, groups, X, Y, single):
        """Rows that do not fit the window any more.  ONE observation into a full window: the rank-one replacement of the oldest row
        in every group, then the ring row is overwritten (in stream order: the replacement has read it) and the slot advances.  Anything
        else: the newest `window` rows, oldest first, become the ring and every group is refitted."""
        w = self._window
        if single and self.num_train == w:
            s = self.window_slot
            xo, yo = self._Xbuf[s:s + 1], self._Ybuf[s:s + 1]
            Ro, Rn = self._residual(xo, yo), self._residual(X, Y)
            for cols, st in groups:
                st.replace(xo[0], Ro[0, cols].contiguous(), X[0], Rn[0, cols].contiguous())
            self._Xbuf[s].copy_(X[0])
            self._Ybuf[s].copy_(Y[0])
            self.window_slot = (s + 1) % w
            self._replacements += 1
            if self.rebase_every and self._replacements >= self.rebase_every:
                Xw, Yw = self._rows()
                Rw = self._residual(Xw, Yw)
                for cols, st in groups:
                    st.rebase(Xw, Rw[:, cols].contiguous())
                self._replacements = 0
            return
        if self.num_train:
            Xo, Yo = self._rows()
            X, Y = torch.cat((Xo, X)), torch.cat((Yo, Y))
        X, Y = X[-w:].contiguous(), Y[-w:].contiguous()
        if self._Xbuf is None:
            self.num_train = 0
            self._store(X[:0], Y[:0])
        self._Xbuf.copy_(X)
        self._Ybuf.copy_(Y)
        self.num_train, self.window_slot, self._replacements = w, 0, 0
        R = self._residual(X, Y)
        for cols, st in groups:
            st.fit(X, R[:, cols].contiguous())

    # -- device pack -------------------------------------------------------------------------------
    def _key(self):
        return [self._data_version, self._z_version] + self._hyper_key() + [self._nominal_key()]

    @staticmethod
    def _same_key(a, b):
        return (a is not None and b is not None and len(a) == len(b) and a[0] == b[0] and a[1] == b[1] and a[-1] == b[-1]
                and SparseDynamics._same_hyper(a[2:-1], b[2:-1]))

    def posterior(self):
        """(alpha (M, ds), Q (M, M) shared or (ds, M, M)) of the current data and hyper-parameters, device tensors."""
        if self.num_train == 0:
            raise RuntimeError("no training data")
        groups = self._ensure_groups()
        if len(groups) == 1:
            cols, st = groups[0]
            if cols == list(range(self.state_dim)):
                return st.alpha, st.Q
        alpha = torch.empty((self.M, self.state_dim), dtype=torch.float64, device=self.device)
        Q = torch.empty((self.state_dim, self.M, self.M), dtype=torch.float64, device=self.device)
        for cols, st in groups:
            for k, a in enumerate(cols):
                alpha[:, a] = st.alpha[:, k]
                Q[a] = st.Q
        return alpha, Q

    def pack(self):
        """The device-resident constants of the rollout: built once from (Z, alpha, Q), refilled in place when data or hypers changed."""
        if self.num_train == 0:
            raise RuntimeError("no training data")
        self._ensure_groups()
        key = self._key()
        if self._pack is None or not self._same_key(key, self._pack_key):
            alpha, Q = self.posterior()
            lam = np.stack([g.get_lambdas() for g in self.gpr_err])
            sf = np.array([g.get_sigma_f() for g in self.gpr_err])
            nominal = self._nominal_arrays()
            if self._pack is None or not self._pack.rebuild(self._Z, alpha, Q, lam, sf, nominal=nominal, y_is_beta=True):
                self._pack = GPPack(self._Z, alpha, Q, lam, sf, device=self.device, y_is_beta=True, nominal=nominal)
            self._pack_key = key
        self._apply_noise(self._pack)
        return self._pack
