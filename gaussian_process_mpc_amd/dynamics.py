"""Dynamics: host-side mirror of the reference class (src/dynamics.py:8-191) -- a bundle of
``state_dim`` GPs sharing X_train -- whose rollout runs in the HIP library.

``forward_propagate_torch`` keeps the reference signature and return types (lists of H+1 tensors, graph
attached when the actions require grad).
The batched entry ``rollout`` is the build's extension (the reference handles one trajectory per call).
"""
import warnings

import numpy as np
import torch

from .gpr import GaussianProcessRegression
from .nominal import LinearNominalModel, stack_linear
from .autograd import RolloutFunction, wants_grad
from .rollout import CostParams, GPPack, noise_arrays, rollout, rollout_fullcov


class Dynamics(object):
    def __init__(self, state_dim, action_dim, nominal_models=None):
        self.state_dim = state_dim
        self.action_dim = action_dim
        self.nominal_models = nominal_models
        if nominal_models is None:
            self.gpr_err = [GaussianProcessRegression(state_dim + action_dim) for _ in range(state_dim)]
        else:
            self.gpr_err = [GaussianProcessRegression(state_dim + action_dim, nominal_models[i])
                            for i in range(state_dim)]
        self.device = self.gpr_err[0].device
        self._pack = None
        self._pack_key = None
        self._nominal_warned = False
        self._noise = None                               # (init_cov, action_var, process_var | "sigma_n") of set_noise_model, or None
        self._noise_applied = None                       # (pack, sigma_n sources) the model was last written to
        # Fixed-size training window (extension; None: the training set grows without bound, as in the reference).  Once num_train has
        # reached max_train, a single new observation REPLACES the row at `window_slot` in every GP (first-in first-out: slot 0 first,
        # the oldest row after a bulk load) and the slot advances modulo max_train.  X_train / y_train of the GPs are then in SLOT
        # order, not chronological order: the rows from `window_slot` on are the older ones.
        self.max_train = None
        self.window_slot = 0

    def append_train_data(self, state, action, next_state, incremental=False, async_rebuild=None, refresh=None):
        """(state, action, next_state) observations, one or many (src/dynamics.py:39-60).  incremental=True: O(N^2)
        update of every Ky_inv for a single new observation (see GaussianProcessRegression.append_train_data);
        async_rebuild (True / False; None leaves the GPs' setting): the periodic full rebuild of the incremental path on a
        side stream instead of on the step that reaches `rebuild_every`; refresh ("rebuild" / "newton"; None leaves the GPs'
        setting): a Newton-Schulz polish of the updated inverse instead of that rebuild (GaussianProcessRegression.refresh).
        With `max_train` set: a single observation that arrives at num_train == max_train replaces row `window_slot` (incremental=True:
        C ABI ``gpmpc_gp_replace``; False: a rebuild on the window's rows); a call that would exceed the budget otherwise keeps the
        newest max_train rows in chronological order, rebuilds and resets the slot to 0."""
        if async_rebuild and self.max_train is not None:
            raise ValueError("max_train (fixed-size window) is not supported together with async_rebuild=True")
        if async_rebuild is not None:
            for g in self.gpr_err:
                g.async_rebuild = bool(async_rebuild)
        if refresh is not None:
            if refresh not in ("rebuild", "newton"):
                raise ValueError("refresh must be 'rebuild' or 'newton', got %r" % (refresh,))
            for g in self.gpr_err:
                g.refresh = refresh
        state, action, next_state = np.asarray(state), np.asarray(action), np.asarray(next_state)
        # Every GP receives the same input rows; GPs whose hyper-parameters are bit-identical then have identical Ky /
        # Ky_inv and share one build (GaussianProcessRegression.update_many).  That only holds while ALL data went through
        # this method: once a GP was fed on its own (its X_train is no longer the tensor left here), each is updated by itself.
        uniform = getattr(self, "_uniform_ok", True)
        if uniform:
            seen = getattr(self, "_seen_X", None)       # the input tensors this method left in the GPs last time
            if seen is None:
                uniform = all(g.num_train == 0 for g in self.gpr_err)
            else:
                uniform = all(g.X_train is sx for g, sx in zip(self.gpr_err, seen))
        self._uniform_ok = uniform                       # once a GP was fed on its own, never again
        if len(state.shape) == 1:
            x = np.concatenate((state, action))
            ys = [next_state[i] for i in range(self.state_dim)]
        else:
            if len(action.shape) == 1:
                action = action[:, None]
            x = np.concatenate((state, action), axis=1)
            ys = [next_state[:, i] for i in range(self.state_dim)]
            incremental = False
        if self.max_train is not None:
            n_new = 1 if len(state.shape) == 1 else x.shape[0]
            n_old = self.gpr_err[0].num_train
            if n_new == 1 and n_old == self.max_train and all(g.num_train == n_old for g in self.gpr_err):
                self._replace_in_window(np.reshape(x, (1, -1)), np.reshape(next_state, (1, self.state_dim)), incremental, uniform)
                return
            if n_old + n_new > self.max_train:
                x, ys = self._trim_to_window(np.reshape(x, (n_new, -1)), np.reshape(next_state, (n_new, self.state_dim)))
                if x is None:                                # the GPs held different rows: each was rebuilt on its own
                    return
                next_state = np.stack(ys, axis=1)
                incremental, uniform = False, True
        if not uniform:
            for g, y in zip(self.gpr_err, ys):
                g.append_train_data(x, y, incremental=incremental)
        else:
            modes = []
            # one device copy of the new input rows and one of ALL targets for the ds GPs (they were 2 ds host-to-device copies)
            # (made on first use: the in-place path of a single observation sends its targets as kernel arguments instead)
            shared = {"y_all_host": np.asarray(next_state, dtype=np.float64).reshape(-1, self.state_dim)}
            for a, (g, y) in enumerate(zip(self.gpr_err, ys)):
                if not np.isscalar(y) and np.ndim(y) > 0:
                    n_obs, yy = len(y), np.asarray(y)[:, None]
                    xx = x
                else:
                    n_obs, yy = 1, np.array([y])[:, None]
                    xx = np.reshape(x, (1, g.x_dim))
                modes.append(g._ingest(xx, yy, n_obs, incremental, shared=shared, column=a))
            GaussianProcessRegression.update_many(self.gpr_err, modes)
        self._seen_X = [g.X_train for g in self.gpr_err]

    # -- fixed-size window -------------------------------------------------------------------
    def _replace_in_window(self, x, y_row, incremental, uniform):
        """One observation into slot `window_slot` of every GP (num_train == max_train), then the slot advances."""
        slot = self.window_slot
        if slot >= self.max_train:
            slot = 0
        if not uniform:
            for a, g in enumerate(self.gpr_err):
                g.replace_train_data(slot, x, y_row[0, a], incremental=incremental)
        else:
            shared = {}
            modes = [g._ingest_replace(slot, x, y_row[0, a], incremental, shared=shared) for a, g in enumerate(self.gpr_err)]
            GaussianProcessRegression.update_many(self.gpr_err, modes)
        self.window_slot = (slot + 1) % self.max_train
        self._seen_X = [g.X_train for g in self.gpr_err]

    def _trim_to_window(self, x_new, y_new):
        """A call that would take the training set beyond max_train: the rows every GP holds, in CHRONOLOGICAL order (slot order rotated
        by window_slot), followed by the new ones; the newest max_train of them are kept and the GPs emptied, so that the caller's bulk
        path rebuilds on exactly those rows.  Rare (a bulk load into a full window): goes through the host."""
        m = int(self.max_train)
        if m < 1:
            raise ValueError("max_train must be a positive number of training points, got %r" % (self.max_train,))
        rows_x, rows_y = [], []
        for a, g in enumerate(self.gpr_err):
            if g.num_train:
                Xg, yg = g.X_train.detach().cpu().numpy(), g.y_train.detach().cpu().numpy().reshape(-1)
                if g.num_train == m and self.window_slot:
                    Xg, yg = np.roll(Xg, -self.window_slot, axis=0), np.roll(yg, -self.window_slot)
                rows_x.append(np.concatenate((Xg, x_new), axis=0)[-m:])
                rows_y.append(np.concatenate((yg, y_new[:, a]))[-m:])
            else:
                rows_x.append(x_new[-m:])
                rows_y.append(y_new[-m:, a])
            g.X_train = g.y_train = g.Kf = g.Ky = g.Ky_inv = None
            g.num_train = 0
            g._beta = None
            g._pending = None
        self.window_slot = 0
        if all(np.array_equal(rx, rows_x[0]) for rx in rows_x[1:]):
            self._uniform_ok, self._seen_X = True, None          # every GP restarts from the same rows: they can share builds again
            return rows_x[0], rows_y
        self._uniform_ok = False
        for g, rx, ry in zip(self.gpr_err, rows_x, rows_y):
            g.append_train_data(rx, ry)
        self._seen_X = [g.X_train for g in self.gpr_err]
        return None, None

    # -- device pack -----------------------------------------------------------------------
    def _key(self):
        # what forward_propagate_torch reads at call time in the reference (src/dynamics.py:150, :170-173):
        # Ky_inv, exp(log_lambdas), y_train, sigma_f of every GP, X_train of GP 0.  Tensors are keyed by OBJECT and
        # autograd version (the key holds the references, so an id cannot be reused by a later tensor): this runs on
        # every solver callback, and exp / tolist of the hyper-parameters per call cost as much as a small rollout.
        # ... and, last, the coefficients of the linear nominal models the rollout adds back (None: no such models)
        return [(g.version, g.num_train, g.log_lambdas, g.log_lambdas._version, g.log_sigma_f, g.log_sigma_f._version)
                for g in self.gpr_err] + [self._nominal_key()]

    def _nominal_key(self):
        ms = self.nominal_models                         # (runs on every solver callback: no array work here)
        if ms is None:
            return None
        if len(ms) == self.state_dim and all(isinstance(m, LinearNominalModel) for m in ms):
            return tuple(m.key for m in ms)
        self._linear_nominal()                           # (warns, once)
        return None

    def _linear_nominal(self):
        """(W, b) when every nominal model is a LinearNominalModel: the rollout then honours them.  Other callables are honoured by the GPs
        only (beta, predictions, hyper-parameter training), as in the reference (src/dynamics.py:64): said once, as a warning."""
        if self.nominal_models is None:
            return None
        lin = stack_linear(self.nominal_models, self.state_dim, self.action_dim)
        if lin is None and not getattr(self, "_nominal_warned", False):
            self._nominal_warned = True
            warnings.warn("Dynamics: the rollout ignores nominal models that are not LinearNominalModel (they enter the GPs' residual "
                          "targets only); its means, variances, cost and gradient are those of the zero-mean GPs", stacklevel=3)
        return lin

    @staticmethod
    def _same_key(a, b):
        if a is None or b is None or len(a) != len(b) or a[-1] != b[-1]:
            return False
        return all(x[0] == y[0] and x[1] == y[1] and x[2] is y[2] and x[3] == y[3] and x[4] is y[4] and x[5] == y[5]
                   for x, y in zip(a[:-1], b[:-1]))

    def pack(self):
        """The device-resident constants of the rollout, rebuilt only when data or hypers changed."""
        key = self._key()
        if self._pack is None or not self._same_key(key, self._pack_key):
            g0 = self.gpr_err[0]
            if g0.num_train == 0:
                raise RuntimeError("no training data")
            Y = torch.cat([g.y_train.reshape(-1, 1) for g in self.gpr_err], dim=1)
            if all(g.Ky_inv is g0.Ky_inv for g in self.gpr_err):
                Kinv = g0.Ky_inv.detach()               # GPs with identical hyper-parameters share ONE inverse: read in place, no stack
            else:
                Kinv = torch.stack([g.Ky_inv.detach() for g in self.gpr_err])
            lam = np.stack([g.get_lambdas() for g in self.gpr_err])
            sf = np.array([g.get_sigma_f() for g in self.gpr_err])
            # the closed loop appends one observation per step: refill the existing pack while its padded size fits
            nominal = self._linear_nominal()            # (Y stays the raw targets: the library removes the linear model on the device)
            if self._pack is None or not self._pack.rebuild(g0.X_train, Y, Kinv, lam, sf, nominal=nominal):
                self._pack = GPPack(g0.X_train, Y, Kinv, lam, sf, device=self.device, nominal=nominal)
            self._pack_key = key
        self._apply_noise(self._pack)
        return self._pack

    # -- noise model (extension) -----------------------------------------------------------
    def set_noise_model(self, init_cov=None, action_var=None, process_var=None):
        """Noise model of every rollout of this object (GPPack.set_noise): init_cov (ds, ds) or a (ds,) diagonal, action_var (da,),
        process_var (ds,) -- or the string "sigma_n": each GP's current sigma_n^2, so that the propagated variance is that of the next
        STATE (Sigma_t+1 = Sigma^f + Sigma_w) rather than of the latent function; it follows later hyper-parameter updates.  None: that
        part's default; all None: the reference's constants.  Stored here and re-applied whenever this object creates a new pack (the
        training set outgrowing its padded size); on the pack that exists it is one small set -- not a rebuild, and not part of the
        rebuild key."""
        follow = isinstance(process_var, str)
        if follow and process_var != "sigma_n":
            raise ValueError('process_var: an array of %d variances or the string "sigma_n", got %r' % (self.state_dim, process_var))
        P, av, pv = noise_arrays(self.state_dim, self.action_dim, init_cov, action_var, None if follow else process_var)
        for name, arr in (("init_cov", P), ("action_var", av), ("process_var", pv)):
            if arr is not None and not np.all(np.isfinite(arr)):
                raise ValueError("%s must be finite" % name)
        self._noise = (P, av, "sigma_n" if follow else pv)
        self._noise_applied = None
        if self._pack is not None:
            self._apply_noise(self._pack)

    def _apply_noise(self, pack):
        """Write the stored model into ``pack`` if it does not hold it yet (runs on every solver callback: identity checks only)."""
        nm = getattr(self, "_noise", None)
        if nm is None:                                   # never set: a pack starts with the defaults
            return
        P, av, pv = nm
        src = tuple((g.log_sigma_n, g.log_sigma_n._version) for g in self.gpr_err) if isinstance(pv, str) else None
        old = getattr(self, "_noise_applied", None)
        if old is not None and old[0] is pack and (src is None or all(a[0] is b[0] and a[1] == b[1] for a, b in zip(src, old[1]))):
            return
        if src is not None:
            pv = np.array([float(g.get_sigma_n()) ** 2 for g in self.gpr_err])
        pack.set_noise(P, av, pv)
        self._noise_applied = (pack, src)

    # -- rollout ---------------------------------------------------------------------------
    def rollout(self, curr_state, actions, cost=None, want_grad=False, full_covariance=False):
        """Batched rollout: curr_state (ds,) or (B, ds); actions (H, da) or (B, H, da).
        Returns the dict of gaussian_process_mpc_amd.rollout.rollout (or rollout_fullcov: 'covs' instead of 'vars')."""
        if cost is None:     # propagation only: a zero cost keeps the fused tail trivial
            cost = CostParams(0.0, np.zeros((self.state_dim, self.state_dim)), np.zeros((self.action_dim, self.action_dim)))
        if full_covariance:
            if self._linear_nominal() is not None:
                raise NotImplementedError("full_covariance=True is not supported with linear nominal models")
            return rollout_fullcov(self.pack(), curr_state, actions, cost, want_grad=want_grad)
        return rollout(self.pack(), curr_state, actions, cost, want_grad=want_grad, want_traj=True)

    def particle_rollout(self, curr_state, actions, particles=1024, seed=0, call_index=0, constraints=None, return_particles=True):
        """Monte-Carlo rollout through the GPs' pointwise posterior (gaussian_process_mpc_amd.particles.particle_rollout): the check of
        what ``rollout`` approximates by moment matching.  Reads the GPs' arrays in place; the pack is not touched."""
        from .particles import particle_rollout
        return particle_rollout(self, curr_state, actions, particles=particles, seed=seed, call_index=call_index, constraints=constraints,
                                return_particles=return_particles)

    def forward_propagate(self, horizon, curr_state, actions):
        """The reference's numpy rollout (src/dynamics.py:62-124; its slow double-loop oracle, sigma_f = 1 only) with the same
        signature and return types -- numpy (H+1, ds) means and (H+1, ds, ds) diagonal covariances -- evaluated by the HIP
        path.  One documented difference: the numpy version adds an action-noise variance of exactly 1e-3, the torch version
        (and this library) float32(1e-3) (src/dynamics.py:162); the reference's own test holds the two to 1e-7
        (src/test/test_dynamics.py:134-196) and so do these values."""
        r = self.rollout(np.asarray(curr_state, dtype=np.float64).reshape(self.state_dim),
                         np.asarray(actions, dtype=np.float64).reshape(horizon, self.action_dim))
        means = r["means"][0].cpu().numpy()
        covars = np.zeros((horizon + 1, self.state_dim, self.state_dim))
        v = r["vars"][0].cpu().numpy()
        for t in range(horizon + 1):
            covars[t] = np.diag(v[t])
        return means, covars

    def forward_propagate_torch(self, horizon, curr_state, actions):
        """Means and (diagonal) covariances of the H-step shooting rollout (src/dynamics.py:126-191).
        Returns (list of H+1 (ds,) tensors, list of H+1 (ds,ds) tensors) on the device.  Like the reference's, the
        tensors carry the autograd graph when ``actions`` (or ``curr_state``) requires grad: the reference pattern
        ``forward_propagate_torch -> cost_torch -> backward()`` (src/mpc.py:217-255) works on the mirror classes; the
        graph has ONE node for the whole rollout (autograd.RolloutFunction: HIP forward, analytic step Jacobians, reverse
        sweep on the device) instead of ~40 torch ops per (step, GP)."""
        U = torch.as_tensor(actions)
        x0 = torch.as_tensor(curr_state)
        if wants_grad(U, x0):
            Ud = U.to(self.device, torch.float64).reshape(1, horizon, self.action_dim)
            xd = x0.to(self.device, torch.float64).reshape(1, self.state_dim)
            means, vars_ = RolloutFunction.apply(xd, Ud, self.pack())
            means, vars_ = means[0], vars_[0]
        else:
            U = U.detach().to(self.device, torch.float64).reshape(horizon, self.action_dim)
            x0 = x0.detach().to(self.device, torch.float64).reshape(self.state_dim)
            r = self.rollout(x0, U)
            means, vars_ = r["means"][0], r["vars"][0]
        return [means[t] for t in range(horizon + 1)], [torch.diag(vars_[t]) for t in range(horizon + 1)]
