"""RiskSensitiveMPC: host-side mirror of the reference class (src/mpc.py:7-330).

The cyipopt problem-object surface is kept (``objective`` / ``gradient`` / ``constraints`` /
``jacobian``), as are the constructor, the setters and ``get_optimal_trajectory``.  Differences, all
forced by moving the rollout into one fused HIP call:

* ``objective(x)`` evaluates cost AND gradient in the same device pass and caches both keyed on the
  bytes of ``x`` (the reference keeps an autograd graph and back-propagates lazily, src/mpc.py:225-255,
  and its ``gradient`` ignores ``x``); Ipopt's buffer is copied, never aliased (src/mpc.py:217).
* ``objective_batch`` / ``evaluate_batch`` evaluate many candidate action sequences at once (the
  trajectory-sharded batch the multi-GPU path consumes) -- an extension, the reference has no batch API.
* ``gamma == 0`` is accepted and means the analytic risk-neutral limit.
* ``get_optimal_trajectory(curr_state, n_starts=K)`` (or ``mpc.n_starts = K``) with K > 1 runs K bounded quasi-Newton searches in
  lock-step (multistart.py): every solver iteration is ONE ``evaluate_batch`` call of K candidate plans -- sharded over the
  ranks when ``torch.distributed`` is initialised -- and the best local optimum is returned.  ``n_starts = 1`` (the default)
  is the reference's single zero-start solve (src/mpc.py:292-326).
* ``set_state_constraints`` / ``set_state_bounds`` (extension; the reference's ``constraints`` returns 0, src/mpc.py:257-267): linear chance
  constraints A mu_t + kappa sd_t <= b on every predicted state.  ``constraints(x)`` / ``jacobian(x)`` then return their values and the
  dense Jacobian from the SAME device pass as cost and gradient (``gpmpc_rollout_constrained``), and the cyipopt problem gets
  m = H m_c rows.  Without constraints set nothing changes.
* ``solver = "mppi"`` (extension; ``mpc.solver`` or ``get_optimal_trajectory(x, solver="mppi")``): the sampling planner of mppi.py -- K
  perturbed copies of the previous plan, shifted by one step, rolled out as one objective-only batch per iteration, the whole search one
  enqueue on the device (``gpmpc_mppi_solve``).  State constraints that are set become its feasibility rule.  ``solver = None`` (the
  default) is everything above, unchanged.
* ``solver = "lbfgs"`` (extension): the lock-step multi-start search with its state machine on the device (device_lbfgs.py,
  ``gpmpc_lbfgs_solve``) -- ``n_starts`` starts from ``make_starts``, options from ``multistart_options`` plus ``check_every``, the ticks
  enqueued without a device-to-host copy in between.  Unconstrained; the diagonal rollout, or the full-covariance one under
  ``propagation = "moment_matching_full"``.
* ``solver = "auglag"`` (extension): the constrained multi-start on the device (device_auglag.py, ``gpmpc_auglag_solve``) -- an augmented
  Lagrangian over the batched constrained rollout with the search above as its inner solver; ``n_starts`` starts, options from
  ``auglag_options``.  Needs state constraints; the diagonal rollout, or the full-covariance one under ``"moment_matching_full"``.
* ``set_reference_trajectory`` / ``mpc.reference = fn`` / ``mpc.Q_terminal`` (extension; the reference measures every step against one
  ``x_ref`` under one ``Q``): references that change along the horizon and a terminal weight, through ONE ``rollout.CostSchedule`` owned
  by the controller.  Its rows live in device memory, so the solver-callback graph of the closed loop is captured once however often
  the window moves.  Every callback, batch evaluation, ``cost_torch`` and solver reads it; with none of the three set nothing changes.
* ``mpc.propagation = "linearised"`` (extension; linearised.py): the first-order propagation mu' = m(z),
  var' = s2(z) + grad m^T S grad m in the place of exact moment matching -- in the four solver callbacks (one B = 1
  ``linearised_rollout`` per x), ``evaluate_batch`` (and with it the host lock-step multi-start) and ``solver = "mppi"``
  (``gpmpc_mppi_solve_linearised``).  ``solver = "lbfgs"``, ``solver = "auglag"`` and ``full_covariance=True`` refuse it (not yet); the
  lock-step multi-start, which replays its batch as a hipGraph under moment matching, issues plain launches instead (the C entry refuses
  ``GPMPC_USE_GRAPH``).  ``"moment_matching"`` (the default) is everything above, unchanged.  ``mpc.linearised_form = "tile" | "stream" |
  "auto"`` hands every one of these calls its ``form=`` (linearised.py: "stream" is the matrix-vector form for the B = 1 callbacks and the
  small batches of the multi-start); ``None``, the default, leaves the process-wide choice alone.
* ``mpc.propagation = "linearised_full"`` (extension): the linearised rule with the WHOLE covariance, predicted
  under the state feedback u_t = v_t + K_t (x_t - mu_t) that ``mpc.set_feedback_gain(K)`` sets (``clear_feedback_gain`` drops it;
  ``linearised.lqr_gain`` makes a stabilising one).  The chance constraints then see a_r^T Sigma_t a_r of a plant that is steered back.
  It serves what ``"linearised"`` serves -- the callbacks, ``evaluate_batch`` (``covs`` in the place of ``vars``), the host lock-step
  multi-start and ``solver = "mppi"`` (a host loop of sample / rollout / update calls), with and without state constraints --;
  ``solver = "lbfgs"`` and ``"auglag"`` refuse it (not yet).  The ``full_covariance`` attribute is not consulted under it, and
  ``"linearised"`` with ``full_covariance=True`` keeps refusing.  A gain under any other propagation raises.
* ``mpc.feedback_input_cost`` / ``set_input_chance_bounds`` / ``set_input_constraints`` (extension; under
  ``"linearised_full"`` only, any other propagation raises): with a gain the commanded input is N(v_t, K_t Sigma_t K_t^T).  The first adds
  sum_t tr(R K_t Sigma_t K_t^T) to the cost; the others add rows c . v_t + kappa sqrt(a^T Sigma_t a) <= d, a = K_t^T c, on the steps
  t = 0..H-1.  ``constraints(x)`` / ``jacobian(x)`` return the state block followed by the input block, ``evaluate_batch(constraints=True)``
  carries ``g_u`` / ``g_u_jac``, ``solver = "mppi"`` honours both; the box lb <= v <= ub of the solvers stays.
  ``validate_plan(feedback=True)`` runs the particles under the gain and reports the inputs' spread and satisfaction.
* ``mpc.propagation = "moment_matching_full"`` (extension): exact moment matching with the WHOLE covariance in every
  path -- the four solver callbacks (one B = 1 ``rollout_fullcov(..., constraints=)`` per x: cost, gradient, g on a_r^T Sigma_t a_r and its
  dense Jacobian from one pass), ``evaluate_batch`` with and without constraints (``covs`` in the place of ``vars``), the unconstrained host
  multi-start, ``solver = "mppi" | "lbfgs" | "auglag"`` (``gpmpc_*_solve_fullcov``) and ``validate_plan`` (``cov_mm``).  The
  ``full_covariance`` attribute is not consulted under it; ``"moment_matching"`` with ``full_covariance=True`` keeps the refusals it had.
  Refused under it: a feedback gain, a nominal model, ``n_starts > 1`` with state constraints and ``solver=None``.
* ``mpc.propagation = "particles"`` (extension; particles.py): no moments at all -- the plan is scored on
  ``mpc.particle_options["particles"]`` Monte-Carlo particles through the GP posterior: the entropic risk of the stage cost over the
  particles and, for the chance constraints, the empirical quantile of every row's margin (kappa = 0 constrains the MEDIAN where the
  Gaussian rule constrains the mean).  It is the distribution ``validate_plan`` checks a moment-matched plan against, and it serves
  nominal models, the noise model, ``SparseDynamics`` and windows.  There are no gradients through particles: ``solver = "mppi"``
  (``gpmpc_mppi_solve_particles``; the seed is ``mppi_options["seed"]``, the call index the solve count, the particle noise the same in
  every iteration of a solve), ``evaluate_batch`` (cost and g, ``grad`` None) and ``objective(x)`` work; ``gradient``, ``jacobian`` and
  every other solver, the default included, raise ``NotImplementedError``.  A feedback gain raises; ``full_covariance`` is not consulted.
"""
import numpy as np
import torch

from .autograd import CostFunction, wants_grad
from .dynamics import Dynamics
from .rollout import CostParams, CostSchedule, InputConstraints, StateConstraints, cost_full, rollout, rollout_fullcov

try:                                    # the solver binding is optional (not installed in the build image)
    import cyipopt                      # noqa: F401
    HAVE_CYIPOPT = True
except Exception:                       # pragma: no cover
    cyipopt = None
    HAVE_CYIPOPT = False


class RiskSensitiveMPC:
    feedback_input_cost = False                          # charge tr(R K Sigma K^T), the spread of the commanded input ("linearised_full" only)
    input_constraints = None                             # rollout.InputConstraints on the commanded input, or None ("linearised_full" only)
    propagation = "moment_matching"                      # | "moment_matching_full" | "linearised" | "linearised_full" | "particles" (extension): which rule the rollouts of the solvers use
    particle_options = {"particles": 256}                # propagation = "particles": particles per plan (1 ... 4096); assign a new dict to change it
    linearised_form = None                               # | "tile" | "stream" | "auto": the form of the linearised step (None: the process-wide one)

    def __init__(self, gamma, horizon, state_dim, input_dim, Q, R, R_delta=None, full_covariance=False, nominal_models=None):
        # nominal_models (extension; the reference passes None, src/mpc.py:45): one callable per state dimension, handed to Dynamics.  A list
        # of LinearNominalModel is honoured by the rollout, the callbacks and the multi-start solve; other callables by the GPs only.
        # full_covariance=True propagates the whole state covariance (off-diagonal terms from the exact
        # cross-covariances): the extension the reference leaves as a TODO (src/dynamics.py:184), BASELINE config 5.
        self.full_covariance = full_covariance
        self.gamma = gamma
        self.horizon = horizon
        self.state_dim = state_dim
        self.input_dim = input_dim
        self.Q = Q
        self.R = R
        self.R_delta = R_delta
        self.dynamics = Dynamics(self.state_dim, self.input_dim, nominal_models=nominal_models)
        self.device = self.dynamics.device
        self.Q_tor = torch.tensor(np.asarray(self.Q), device=self.device).type(torch.float64)
        self.R_tor = torch.tensor(np.asarray(self.R), device=self.device).type(torch.float64)
        self.R_delta_tor = (torch.tensor(np.asarray(self.R_delta), device=self.device).type(torch.float64)
                            if self.R_delta is not None else None)
        self.x_ref = torch.zeros(self.state_dim, device=self.device)
        self.u_ref = torch.zeros(self.input_dim, device=self.device)
        self.curr_cost = None
        self.curr_grad = None
        self.curr_state = None
        self.backward_taken = False
        self.curr_u = None
        self._cache_key = None
        self.last_traj = np.random.standard_normal(size=(self.horizon * self.input_dim,))   # src/mpc.py:62
        self.ub = [1e16 for _ in range(self.input_dim)]
        self.lb = [-1e16 for _ in range(self.input_dim)]
        self.train_empty = True
        self.solver_used = None
        # lock-step multi-start solve (extension; multistart.py): K starts, tick budget, seed of the sampled starts
        self.n_starts = 1
        self.multistart_options = {"max_ticks": 150, "history": 6, "gtol": 1e-4, "ftol": 1e-10, "spread": 1.0, "seed": 0, "warm": True,
                                   "patience": 8, "line_points": 4}      # 4 step lengths per start and tick: one batch of 4 K plans
        self.last_solve_info = None
        self._solve_count = 0
        self.state_constraints = None                    # rollout.StateConstraints, or None (the reference's unconstrained problem)
        # sampling planner (extension; mppi.py): None = the solvers above | "mppi" | "lbfgs" (device_lbfgs.py, options: multistart_options).  sigma None: a quarter of the box width of each input,
        # 1 along an unbounded one; the seed and the solve count (the call index) fix every sample
        self.solver = None
        self.mppi_options = {"samples": 64, "iterations": 30, "sigma": None, "decay": 0.9, "beta": 0.1, "seed": 0}
        # constrained multi-start on the device (extension; device_auglag.py): the keyword options of auglag_solve
        self.auglag_options = {"outer": 8, "inner_ticks": 25, "rho0": 10.0, "growth": 10.0, "shrink": 0.25, "rho_max": 1e8, "lam_max": 1e12,
                               "feas_tol": 1e-4, "history": 8, "gtol": 1e-6, "ftol": 1e-12, "check_outer": 1}
        self.curr_g = None
        self.curr_g_jac = None
        # time-varying references and terminal weight (extension; rollout.CostSchedule).  Q_terminal: (ds, ds) or None, with or without a
        # reference trajectory (without one the schedule repeats x_ref / u_ref).  reference: None, or fn(k) -> X_ref (H+1, ds) or
        # (X_ref, U_ref), asked for the window of step k = step_index before every solve; step_index counts get_optimal_trajectory calls.
        self.Q_terminal = None
        self.reference = None
        self.step_index = 0
        self._ref_traj = None
        self._sched = None                               # the CostSchedule, created by the first solve that needs one
        self._sched_sig = None                           # what it holds: (versions, sources), see _active_schedule

    # -- reference trajectory and terminal weight (extension)
    def set_reference_trajectory(self, X_ref, U_ref=None, Q_terminal=None):
        """References of the next solves: X_ref (H+1, ds) for the predicted states 0..H, U_ref (H, da) or None = zeros.  Q_terminal, if
        given, also sets ``mpc.Q_terminal``.  ``x_ref`` / ``u_ref`` are ignored while a trajectory is set."""
        X = np.array(X_ref, dtype=np.float64).reshape(self.horizon + 1, self.state_dim)
        U = None if U_ref is None else np.array(U_ref, dtype=np.float64).reshape(self.horizon, self.input_dim)
        if not (np.all(np.isfinite(X)) and (U is None or np.all(np.isfinite(U)))):
            raise ValueError("the reference trajectory must be finite")
        self._ref_traj = (X, U)
        if Q_terminal is not None:
            self.Q_terminal = Q_terminal
        self._cache_key = None

    def clear_reference_trajectory(self):
        """Back to ``x_ref`` / ``u_ref`` (``Q_terminal`` and ``reference`` are attributes: set them to None to drop them)."""
        self._ref_traj = None
        self._cache_key = None

    def _active_schedule(self):
        """The controller's ONE cost schedule with the current references written into it, or None when neither a reference trajectory
        nor a terminal weight is set.  Rewritten (in stream order, same device buffer) only when what it holds has changed: sources are
        compared by identity and tensor version, as ``_cost_params`` compares Q and R -- assign a new ``Q_terminal`` rather than writing
        into the array it holds.  (Attributes are read with a default: the class is also built without its constructor.)"""
        traj, Qt = getattr(self, "_ref_traj", None), getattr(self, "Q_terminal", None)
        if traj is None and Qt is None:
            return None
        H, ds, da = self.horizon, self.state_dim, self.input_dim
        srcs = (traj, Qt) if traj is not None else (self.x_ref, self.u_ref, Qt)
        vers = tuple(t._version if isinstance(t, torch.Tensor) else None for t in srcs)
        sched, old = getattr(self, "_sched", None), getattr(self, "_sched_sig", None)
        if sched is None:
            sched = self._sched = CostSchedule(H, ds, da, device=self.device)
        if old is None or old[0] != vers or len(old[1]) != len(srcs) or any(x is not y for x, y in zip(old[1], srcs)):
            to_np = lambda t: t.detach().cpu().numpy().astype(np.float64) if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)  # noqa: E731
            if traj is not None:
                X, U = traj
            else:
                X, U = np.tile(to_np(self.x_ref).reshape(1, ds), (H + 1, 1)), np.tile(to_np(self.u_ref).reshape(1, da), (H, 1))
            sched.set(X, U, None if Qt is None else np.ascontiguousarray(to_np(Qt)).reshape(ds, ds))
            self._sched_sig = (vers, srcs)                   # (the sources are kept alive: `is` cannot alias later objects)
            self._cache_key = None
        return sched

    # -- sparse GP dynamics (extension; sparse.py)
    def use_inducing_points(self, Z, jitter=None, keep_data=True, window=None):
        """Replace ``self.dynamics`` by a :class:`SparseDynamics` on the inducing points Z (M, state_dim + input_dim): FITC sparse GPs whose
        rollout cost depends on M, not on the number of observations.  The hyper-parameters, nominal models and noise model of the
        current dynamics are taken over; its training data is not (feed the new object).  ``window``: the model holds the newest
        ``window`` observations only (``SparseDynamics(window=...)``).  Returns the new dynamics."""
        from .sparse import SparseDynamics
        old = self.dynamics
        new = SparseDynamics(self.state_dim, self.input_dim, Z, nominal_models=old.nominal_models, jitter=jitter, keep_data=keep_data,
                             window=window)
        for g_new, g_old in zip(new.gpr_err, old.gpr_err):
            g_new.log_lambdas, g_new.log_sigma_f, g_new.log_sigma_n = g_old.log_lambdas, g_old.log_sigma_f, g_old.log_sigma_n
        nm = getattr(old, "_noise", None)
        if nm is not None:
            new.set_noise_model(init_cov=nm[0], action_var=nm[1], process_var=nm[2])
        self.dynamics = new
        self._cache_key = None
        return new

    # -- noise model (extension)
    def set_noise_model(self, init_cov=None, action_var=None, process_var=None):
        """Noise model of the prediction (Dynamics.set_noise_model): covariance of the start state, variance of each input, and a process
        variance added to every predicted state (an array, or "sigma_n" for the GPs' own noise).  Every solver and callback follows it,
        under ``full_covariance=True`` with the whole ``init_cov`` matrix, else with its diagonal."""
        self.dynamics.set_noise_model(init_cov=init_cov, action_var=action_var, process_var=process_var)
        self._cache_key = None

    def set_initial_covariance(self, P):
        """The per-solve call of an estimator-driven loop: the covariance of the state handed to the next ``get_optimal_trajectory``
        ((ds, ds), or a (ds,) diagonal); the other parts of the model stay.  One small device copy: captured graphs are replayed."""
        nm = getattr(self.dynamics, "_noise", None) or (None, None, None)
        self.dynamics.set_noise_model(init_cov=P, action_var=nm[1], process_var=nm[2])
        self._cache_key = None

    # -- setters (src/mpc.py:72-116)
    def set_ub(self, ub):
        assert len(ub) == self.input_dim
        self.ub = ub

    def set_lb(self, lb):
        assert len(lb) == self.input_dim
        self.lb = lb

    def set_xref(self, x_ref):
        assert len(x_ref) == self.state_dim
        self.x_ref = torch.tensor(np.asarray(x_ref), device=self.device).type(torch.float64)
        self._cache_key = None

    def set_uref(self, u_ref):
        assert len(u_ref) == self.input_dim
        self.u_ref = torch.tensor(np.asarray(u_ref), device=self.device).type(torch.float64)
        self._cache_key = None

    # -- state chance constraints (extension)
    def set_state_constraints(self, A, b, prob=None, kappa=None):
        """Rows A[r] . mu_t + kappa[r] sd_t[r] <= b[r] on every predicted state t = 1..H (rollout.StateConstraints: exactly one of
        ``prob`` -- one-sided satisfaction probability -- and ``kappa``)."""
        sc = StateConstraints(A, b, kappa=kappa, prob=prob)
        if sc.ds != self.state_dim:
            raise ValueError("constraint rows must have one coefficient per state dimension")
        self.state_constraints = sc
        self._cache_key = None

    def set_state_bounds(self, lb, ub, prob):
        """Chance bounds lb[k] <= x_k <= ub[k], each held with probability ``prob``; None / +-inf entries are unbounded."""
        self.state_constraints = StateConstraints.box(lb, ub, self.state_dim, prob=prob)
        self._cache_key = None

    def clear_state_constraints(self):
        self.state_constraints = None
        self.curr_g = self.curr_g_jac = None
        self._cache_key = None

    # -- cost
    def _cost_params(self, x_ref=None, u_ref=None):
        xr = self.x_ref if x_ref is None else x_ref
        ur = self.u_ref if u_ref is None else u_ref
        last_u = np.asarray(self.last_traj, dtype=np.float64)[0:self.input_dim] if self.R_delta is not None else None
        # rebuilt only when one of its inputs changes: the solver calls this once per callback and the device-to-host
        # copies of x_ref / u_ref alone cost as much as a small rollout
        sched = self._active_schedule()                           # (its CONTENTS are not part of the key: they live on the device)
        objs = (self.Q, self.R, self.R_delta, xr, ur, sched)      # kept alive by the cache: `is` cannot alias new objects
        vers = tuple(t._version if isinstance(t, torch.Tensor) else None for t in objs)
        key = (self.gamma, vers, None if last_u is None else last_u.tobytes())
        old = getattr(self, "_cp_state", None)
        if old is None or old[0] != key or any(a is not b for a, b in zip(old[1], objs)):
            to_np = lambda t: t.detach().cpu().numpy().astype(np.float64) if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)  # noqa: E731
            self._cp = CostParams(self.gamma, self.Q, self.R, R_delta=self.R_delta, x_ref=to_np(xr), u_ref=to_np(ur),
                                  last_u=last_u, schedule=sched)
            self._cp_state = (key, objs)
        return self._cp

    def cost(self, x, u, sig, x_ref, u_ref):
        """numpy risk-sensitive cost, no input-rate term (src/mpc.py:118-154); host arithmetic in the
        reference too."""
        Q, R, g = np.asarray(self.Q, dtype=float), np.asarray(self.R, dtype=float), self.gamma
        Qi = np.linalg.inv(Q)
        eye = np.identity(self.state_dim)
        total = 0
        for i in range(self.horizon + 1):
            e = x[i, :] - x_ref
            total += np.log(np.linalg.det(eye + g * Q @ sig[i, :, :])) / g
            total += e.T @ np.linalg.inv(Qi + g * sig[i, :, :]) @ e
        for j in range(self.horizon):
            d = u[j, :] - u_ref
            total += d.T @ R @ d
        return total

    def cost_torch(self, x, u, sig, x_ref, u_ref):
        """Risk-sensitive cost incl. the input-rate term for FULL covariance matrices
        (src/mpc.py:156-200) on the device; x / sig may be lists of tensors or stacked tensors.  Differentiable
        like the reference's: if any of x, sig, u carries a graph the result does too (autograd.CostFunction), so
        ``cost_torch(...).backward()`` fills ``u.grad`` as src/mpc.py:251 does.  With a reference trajectory or a terminal weight set the
        controller's schedule applies (x has horizon + 1 rows at most) and ``x_ref`` / ``u_ref`` are ignored."""
        xs = torch.stack([t.reshape(-1) for t in x]) if isinstance(x, (list, tuple)) else torch.as_tensor(x)
        ss = torch.stack(list(sig)) if isinstance(sig, (list, tuple)) else torch.as_tensor(sig)
        ss = ss.reshape(xs.shape[0], self.state_dim, self.state_dim)
        xs = xs.reshape(-1, self.state_dim)
        ut = torch.as_tensor(u).reshape(-1, self.input_dim)
        cp = self._cost_params(x_ref, u_ref)
        if wants_grad(xs, ss, ut):
            to = lambda t: t.to(self.device, torch.float64)  # noqa: E731
            return CostFunction.apply(to(xs)[None], to(ss)[None], to(ut)[None], cp)[0]
        return cost_full(cp, xs, ss, ut)[0]

    # -- propagation rule (extension)
    def _linearised(self):
        """True under ``propagation = "linearised"``, after the refusals every entry shares."""
        prop = self.propagation
        if prop not in ("moment_matching", "moment_matching_full", "linearised", "linearised_full", "particles"):
            raise ValueError("propagation must be 'moment_matching', 'moment_matching_full', 'linearised', 'linearised_full' or 'particles', "
                             "got %r" % (prop,))
        if prop == "linearised" and self.full_covariance:
            raise NotImplementedError("propagation='linearised' is diagonal: a full-covariance linearised rollout is not implemented (not yet)")
        if getattr(self, "_feedback_gain", None) is not None and prop != "linearised_full":
            raise ValueError("a feedback gain is set (set_feedback_gain): only propagation='linearised_full' predicts under state feedback, "
                             "got propagation=%r (clear_feedback_gain drops it)" % (prop,))
        if (self.feedback_input_cost or self.input_constraints is not None) and prop != "linearised_full":
            raise ValueError("an input cost or input chance constraints under feedback are set (feedback_input_cost, set_input_constraints / "
                             "set_input_chance_bounds): only propagation='linearised_full' knows the spread of the commanded input, got "
                             "propagation=%r (clear_input_constraints / feedback_input_cost = False drop them)" % (prop,))
        if prop == "moment_matching_full" and getattr(self.dynamics, "nominal_models", None) is not None:
            raise NotImplementedError("propagation='moment_matching_full' with a nominal model: the full-covariance rollout does not know "
                                      "the cross-covariances between a nominal model and the GPs")
        return prop in ("linearised", "linearised_full")

    def _mm_full(self):
        """True under ``propagation = "moment_matching_full"``: every rollout is the full-covariance one, constraints included."""
        return self.propagation == "moment_matching_full"

    def _lin_kw(self):
        """The keyword arguments that select the rule of ``linearised_rollout`` / ``mppi_solve_linearised``."""
        if self.propagation == "linearised_full":
            return {"full_covariance": True, "feedback": getattr(self, "_feedback_gain", None),
                    "input_cost": bool(self.feedback_input_cost), "input_constraints": self.input_constraints}
        return {}

    # -- the commanded input under feedback (extension; propagation = "linearised_full" only)
    def set_input_constraints(self, C, d, prob=None, kappa=None):
        """Rows C[r] . v_t + kappa[r] sqrt(a^T Sigma_t a) <= d[r], a = K_t^T C[r], on the commanded input u_t = v_t + K_t (x_t - mu_t) of
        every step t = 0..H-1 (rollout.InputConstraints: exactly one of ``prob`` and ``kappa``).  The box lb <= v <= ub of the solvers
        stays as it is."""
        ic = InputConstraints(C, d, kappa=kappa, prob=prob)
        if ic.da != self.input_dim:
            raise ValueError("the input constraint rows have %d coefficients, the problem has %d inputs" % (ic.da, self.input_dim))
        self.input_constraints = ic
        self._cache_key = None

    def set_input_chance_bounds(self, prob):
        """Input chance constraints from the finite entries of ``lb`` / ``ub``: P(lb_j <= u_j <= ub_j) >= prob per bound and step."""
        big = 1e15                                                        # (the setters' "no bound")
        lb = [None if v <= -big else float(v) for v in self.lb]
        ub = [None if v >= big else float(v) for v in self.ub]
        self.input_constraints = InputConstraints.box(lb, ub, self.input_dim, prob=prob)
        self._cache_key = None

    def clear_input_constraints(self):
        self.input_constraints = None
        self._cache_key = None

    def _rows(self):
        """(m_c, m_u): the state and the input rows per step that the callbacks stack."""
        sc, ic = self.state_constraints, self.input_constraints
        return (0 if sc is None else sc.m), (0 if ic is None else ic.m)

    def _fullcov_mm(self):
        """``full_covariance`` as the paths that refuse it read it: under "linearised_full" and "moment_matching_full" the attribute is
        not consulted."""
        return bool(self.full_covariance) and self.propagation not in ("linearised_full", "moment_matching_full", "particles")

    def set_feedback_gain(self, K):
        """The gain of the predicted input u_t = v_t + K_t (x_t - mu_t) under ``propagation = "linearised_full"``: (da, ds) for every step or
        (H, da, ds).  It is held as a device tensor (``feedback_gain``): writing into it in place changes the next prediction.  With any
        other propagation every evaluation raises until ``clear_feedback_gain``.  ``lqr_gain`` makes a stabilising one."""
        K = torch.as_tensor(np.asarray(K, dtype=np.float64), device=self.device)
        if tuple(K.shape) not in ((self.input_dim, self.state_dim), (self.horizon, self.input_dim, self.state_dim)):
            raise ValueError("feedback gain: (%d, %d) or (%d, %d, %d), got %s" % (self.input_dim, self.state_dim, self.horizon, self.input_dim,
                                                                                   self.state_dim, tuple(K.shape)))
        if not bool(torch.isfinite(K).all()):
            raise ValueError("feedback gain: non-finite entries")
        self._feedback_gain = K.contiguous()
        self._cache_key = None

    def clear_feedback_gain(self):
        self._feedback_gain = None
        self._cache_key = None

    @property
    def feedback_gain(self):
        return getattr(self, "_feedback_gain", None)

    # -- propagation = "particles" (extension)
    def _particles(self):
        """True under ``propagation = "particles"``."""
        return self.propagation == "particles"

    def _particles_refuse(self, what):
        raise NotImplementedError("propagation='particles' has no gradients through particles: %s is not available -- use solver='mppi' "
                                  "(mppi_solve_particles), evaluate_batch or objective" % (what,))

    def _particle_kw(self):
        """particles / seed / call index of every particle evaluation: ``particle_options``, ``mppi_options["seed"]`` and the solve count
        (the call index the NEXT solve uses, so an evaluation between two solves sees the noise of the coming one)."""
        return {"particles": int(self.particle_options.get("particles", 256)), "seed": int(self.mppi_options.get("seed", 0)),
                "call_index": self._solve_count}

    def _particle_evaluate(self, U, cs, constraints):
        from .particles import particle_evaluate
        r = particle_evaluate(self._linearised_model(self.dynamics.pack()), cs, U, self._cost_params(),
                              constraints=self.state_constraints if constraints else None, **self._particle_kw())
        r["grad"] = None
        return r

    def _linearised_model(self, pack):
        """The dynamics as a ``particles.GPModel``, rebuilt when the pack or the noise model has changed."""
        from .particles import GPModel
        nm = getattr(self.dynamics, "_noise", None)
        held = getattr(self, "_lin_model", None)
        if held is None or held[0] is not pack or held[1] != pack.generation or held[2] is not nm:
            held = self._lin_model = (pack, pack.generation, nm, GPModel.from_dynamics(self.dynamics))
        return held[3]

    # -- cyipopt problem object (src/mpc.py:202-267)
    def _evaluate(self, x):
        x = np.array(x, dtype=np.float64, copy=True).reshape(-1)
        cs, pack, cp = self.curr_state, self.dynamics.pack(), self._cost_params()
        lin = self._linearised()
        fb = getattr(self, "_feedback_gain", None)
        mmf = self._mm_full()
        key = (x.tobytes(), None if cs is None else cs._version, bool(self.full_covariance), pack.generation,
               self.propagation if (lin or mmf) else lin,
               self.linearised_form if lin else None, None if fb is None else (id(fb), fb._version))
        held = getattr(self, "_cache_held", (None, None, None))    # kept alive so that `is` cannot alias later objects
        sc = self.state_constraints
        if sc is not None:
            if self._fullcov_mm():
                raise NotImplementedError("state constraints under the full-covariance rollout are not implemented "
                                          "(q = a^T Sigma_t a and that path's Jacobian layout: a follow-up)")
            key = key + (id(sc),)
        ic = self.input_constraints
        if lin and (ic is not None or self.feedback_input_cost):
            key = key + (None if ic is None else id(ic), bool(self.feedback_input_cost))
        if key != self._cache_key or cs is not held[0] or pack is not held[1] or cp is not held[2]:
            if lin:
                # one B = 1 linearised rollout per x: cost, gradient and, with constraints, g and its dense Jacobian from the same pass
                from .linearised import linearised_rollout
                r = linearised_rollout(self._linearised_model(pack), cs, x.reshape(1, self.horizon, self.input_dim), cp, want_grad=True,
                                       want_traj=False, constraints=sc, form=self.linearised_form, **self._lin_kw())
                self.curr_cost = float(r["cost"][0].item())
                self.curr_grad = r["grad"][0].cpu().numpy()
                if sc is not None:
                    self.curr_g = r["g"][0].cpu().numpy().reshape(-1)
                    self.curr_g_jac = r["g_jac"][0].cpu().numpy()
                if ic is not None:                                        # the state block, then the input block
                    gu, guj = r["g_u"][0].cpu().numpy().reshape(-1), r["g_u_jac"][0].cpu().numpy()
                    self.curr_g = gu if sc is None else np.concatenate([self.curr_g, gu])
                    self.curr_g_jac = guj if sc is None else np.concatenate([self.curr_g_jac, guj], axis=0)
            elif mmf:
                # one B = 1 full-covariance rollout per x: cost, gradient and, with constraints, g on a^T Sigma_t a and its dense Jacobian
                r = rollout_fullcov(pack, cs, x.reshape(1, self.horizon, self.input_dim), cp, want_grad=True, constraints=sc)
                self.curr_cost = float(r["cost"][0].item())
                self.curr_grad = r["grad"][0].cpu().numpy()
                if sc is not None:
                    self.curr_g = r["g"][0].cpu().numpy().reshape(-1)
                    self.curr_g_jac = r["g_jac"][0].cpu().numpy()
            elif sc is not None:
                # ONE device pass for Ipopt's four callbacks on one x: cost, gradient, g and its dense Jacobian
                r = rollout(pack, cs, x.reshape(1, self.horizon, self.input_dim), cp, want_grad=True, want_traj=False, constraints=sc)
                self.curr_cost = float(r["cost"][0].item())
                self.curr_grad = r["grad"][0].cpu().numpy()
                self.curr_g = r["g"][0].cpu().numpy().reshape(-1)
                self.curr_g_jac = r["g_jac"][0].cpu().numpy()
            elif self.full_covariance:
                r = rollout_fullcov(pack, cs, x.reshape(self.horizon, self.input_dim), cp, want_grad=True)
                self.curr_cost = float(r["cost"][0].item())
                self.curr_grad = r["grad"][0].cpu().numpy()
            else:
                # B = 1 is pure latency: upload, the H + 1 kernels and the download are ONE captured hipGraph owned by the
                # pack (C ABI gpmpc_objective_gradient) -- one launch and one wait per callback pair
                # host copy of the state, keyed on ITS OWN source tensor + version (the full-covariance branch also
                # refreshes _cache_held, so that cannot vouch for this copy)
                if getattr(self, "_cs_host_src", None) is not cs or getattr(self, "_cs_host_version", None) != cs._version:
                    self._cs_host = cs.detach().cpu().numpy().astype(np.float64).reshape(-1)
                    self._cs_host_src, self._cs_host_version = cs, cs._version
                cg = pack.objective_gradient(self._cs_host, x.reshape(self.horizon, self.input_dim), cp)
                self.curr_cost = float(cg[0])
                self.curr_grad = cg[1:].reshape(self.horizon, self.input_dim).copy()
            self.curr_u = x.reshape(self.horizon, self.input_dim)
            self.backward_taken = True
            self._cache_key = key
            self._cache_held = (cs, pack, cp)
        return self.curr_cost, self.curr_grad

    def objective(self, x):
        if self._particles():
            self._linearised()
            x = np.array(x, dtype=np.float64, copy=True).reshape(1, self.horizon, self.input_dim)
            return float(self._particle_evaluate(x, self.curr_state, False)["cost"][0].item())
        return self._evaluate(x)[0]

    def gradient(self, x):
        """d cost / d U, shape (horizon, input_dim) like the reference (cyipopt flattens it)."""
        if self._particles():
            self._particles_refuse("gradient")
        return self._evaluate(x)[1]

    def constraints(self, x):
        """0 without state constraints (src/mpc.py:257-262); else g flattened to (H m_c,), row (t-1) m_c + r, feasible where <= 0."""
        if self.state_constraints is None and self.input_constraints is None:
            return 0
        if self._particles():
            self._linearised()
            x = np.array(x, dtype=np.float64, copy=True).reshape(1, self.horizon, self.input_dim)
            return self._particle_evaluate(x, self.curr_state, True)["g"][0].cpu().numpy().reshape(-1)
        self._evaluate(x)
        return self.curr_g

    def jacobian(self, x):
        """Zeros without state constraints (src/mpc.py:264-267); else the dense (H m_c, H da) Jacobian flattened row-major (cyipopt's
        default dense structure)."""
        if self._particles():
            self._particles_refuse("jacobian")
        if self.state_constraints is None and self.input_constraints is None:
            return np.zeros(x.shape)
        self._evaluate(x)
        return self.curr_g_jac.reshape(-1)

    # -- batched evaluation (extension)
    def evaluate_batch(self, U, curr_state=None, want_grad=True, constraints=False):
        """U: (B, H, da) candidates from one (ds,) or per-candidate (B, ds) start state.
        Returns the rollout dict (device tensors: cost (B,), grad (B,H,da), means, vars).
        constraints=True: also g (B, H, m_c) and, with want_grad, g_jac (B, H m_c, H da) of the state constraints that are set."""
        cs = self.curr_state if curr_state is None else curr_state
        lin = self._linearised()
        lin_full = self.propagation == "linearised_full"
        if constraints and self.state_constraints is None and self.input_constraints is None:
            raise ValueError("no state constraints are set (set_state_constraints / set_state_bounds)")
        if self._particles():                                             # cost (B,), stage (B, H+1), g (B, H, m_c) or None, grad None
            return self._particle_evaluate(U, cs, constraints)
        if lin:
            from .linearised import linearised_rollout
            return linearised_rollout(self._linearised_model(self.dynamics.pack()), cs, U, self._cost_params(), want_grad=want_grad,
                                      want_traj=True, constraints=self.state_constraints if constraints else None, form=self.linearised_form,
                                      **dict(self._lin_kw(), **({} if constraints or not lin_full else {"input_constraints": None})))
        if self._mm_full():
            return rollout_fullcov(self.dynamics.pack(), cs, U, self._cost_params(), want_grad=want_grad,
                                   constraints=self.state_constraints if constraints else None)
        if constraints:
            if self.full_covariance:
                raise NotImplementedError("state constraints under the full-covariance rollout are not implemented")
            return rollout(self.dynamics.pack(), cs, U, self._cost_params(), want_grad=want_grad, want_traj=True,
                           constraints=self.state_constraints)
        if self.full_covariance:
            return rollout_fullcov(self.dynamics.pack(), cs, U, self._cost_params(), want_grad=want_grad)
        return rollout(self.dynamics.pack(), cs, U, self._cost_params(), want_grad=want_grad, want_traj=True)

    def objective_batch(self, U, curr_state=None):
        r = self.evaluate_batch(U, curr_state)
        return r["cost"].cpu().numpy(), r["grad"].cpu().numpy()

    # -- Monte-Carlo check of the moment-matched plan (extension)
    def validate_plan(self, U=None, x0=None, particles=4096, seed=0, linearised=False, feedback=False):
        """Compare the moment-matched rollout of a plan (the last one by default; diagonal or full by ``self.full_covariance``, full under ``propagation = "moment_matching_full"``) with a
        particle rollout through the same GPs (``particles.particle_rollout``).  Returns a dict of host arrays:

        ``mean_mm``, ``var_mm`` / ``mean_mc``, ``var_mc`` (H+1, ds): both sets of moments (``cov_mm`` / ``cov_mc`` (H+1, ds, ds) too where the
        rollout is full); ``z_mean``, ``z_var`` (H+1, ds): (Monte-Carlo - moment-matched) in units of the Monte-Carlo standard error,
        sqrt(var / P) for the mean and sqrt((m4 - var^2) / P) for the variance, both from the particles (0 where the error is 0);
        ``clamped`` (H,): particles whose latent variance came out negative; ``stage_cost``: the mean over particles of
        sum_t (x_t - x_ref)^T Q (x_t - x_ref) + sum_t (u_t - u_ref)^T R (u_t - u_ref) (torch, from the particles);
        with state constraints ``satisfaction`` (H, rows), the fraction of particles with a . x_t <= b at t = 1..H, next to
        ``requested`` (rows,) = Phi(kappa), and ``joint_satisfaction``, the fraction satisfying every row at every step.
        With at most 4096 particles also what ``propagation = "particles"`` optimises, from ``particles.particle_cost`` on the same
        particles: ``cost_mc``, ``stage_mc`` (H+1,) and, with state constraints, ``g_mc`` (H, rows).
        linearised=True adds the third column: ``mean_lin``, ``var_lin`` (H+1, ds) of the linearised rollout (linearised.py) and
        ``z_mean_lin``, ``z_var_lin``, its distance from the particles in the same Monte-Carlo standard errors.
        feedback=True (needs ``set_feedback_gain``): the particles run under the gain, u = U_t + K_t (x - mean_lf_t), around the mean
        trajectory of the ``"linearised_full"`` rollout of the plan (``gpmpc_particle_rollout_feedback``), and ``stage_cost`` uses each
        particle's own inputs.  New keys: ``mean_lf`` (H+1, ds), ``cov_lf`` (H+1, ds, ds), ``input_cov_lf`` (H, da, da) = K Sigma K^T,
        ``input_mean_mc`` (H, da), ``input_cov_mc`` (H, da, da) and, with input rows set, ``input_satisfaction`` (H, m_u), the fraction of
        particles with c . u_t <= d at t = 0..H-1, ``input_requested`` (m_u,) and ``joint_input_satisfaction``."""
        from statistics import NormalDist
        from .particles import particle_rollout
        H, ds, da = self.horizon, self.state_dim, self.input_dim
        U = np.asarray(self.last_traj if U is None else U, dtype=np.float64).reshape(H, da)
        cs = self.curr_state if x0 is None else x0
        if cs is None:
            raise ValueError("no start state: give x0 or solve once")
        cs = np.asarray(cs.detach().cpu().numpy() if isinstance(cs, torch.Tensor) else cs, dtype=np.float64).reshape(ds)
        full = bool(self.full_covariance) or self._mm_full()
        mm = self.dynamics.rollout(cs, U, full_covariance=full)
        sc = self.state_constraints
        fb_kw, lf, Kfb = {}, None, getattr(self, "_feedback_gain", None)
        if feedback:
            from .linearised import linearised_rollout
            if Kfb is None:
                raise ValueError("validate_plan(feedback=True) needs a feedback gain (set_feedback_gain)")
            lf = linearised_rollout(self.dynamics, cs, U, None, want_grad=False, form=self.linearised_form, full_covariance=True, feedback=Kfb)
            fb_kw = {"feedback": Kfb, "mean_ref": lf["means"], "input_constraints": self.input_constraints}
        mc = particle_rollout(self.dynamics, cs, U, particles=particles, seed=seed, constraints=sc, **fb_kw)
        P = int(particles)
        X = mc["particles"][0]                                            # (P, H+1, ds)
        out = {"particles": P, "mean_mm": mm["means"][0].cpu().numpy(), "mean_mc": mc["mean"][0].cpu().numpy()}
        cov_mc = mc["cov"][0]
        if full:
            out["cov_mm"], out["cov_mc"] = mm["covs"][0].cpu().numpy(), cov_mc.cpu().numpy()
            out["var_mm"] = np.diagonal(out["cov_mm"], axis1=1, axis2=2).copy()
        else:
            out["var_mm"] = mm["vars"][0].cpu().numpy()
        out["var_mc"] = torch.diagonal(cov_mc, dim1=1, dim2=2).cpu().numpy().copy()
        d = X - mc["mean"][0][None]
        m4 = (d ** 4).mean(dim=0).cpu().numpy()
        se_mean = np.sqrt(np.maximum(out["var_mc"], 0.0) / P)
        se_var = np.sqrt(np.maximum(m4 - out["var_mc"] ** 2, 0.0) / P)
        with np.errstate(divide="ignore", invalid="ignore"):
            out["z_mean"] = np.where(se_mean > 0, (out["mean_mc"] - out["mean_mm"]) / se_mean, 0.0)
            out["z_var"] = np.where(se_var > 0, (out["var_mc"] - out["var_mm"]) / se_var, 0.0)
        out["se_mean"], out["se_var"] = se_mean, se_var
        if linearised:
            from .linearised import linearised_rollout
            ln = linearised_rollout(self.dynamics, cs, U, None, want_grad=False, form=self.linearised_form)
            out["mean_lin"], out["var_lin"] = ln["means"][0].cpu().numpy(), ln["vars"][0].cpu().numpy()
            with np.errstate(divide="ignore", invalid="ignore"):
                out["z_mean_lin"] = np.where(se_mean > 0, (out["mean_mc"] - out["mean_lin"]) / se_mean, 0.0)
                out["z_var_lin"] = np.where(se_var > 0, (out["var_mc"] - out["var_lin"]) / se_var, 0.0)
        out["clamped"] = mc["clamped"][0].cpu().numpy()
        Ud = torch.as_tensor(U, device=X.device)
        ex, eu = X - self.x_ref.to(X.device, torch.float64), Ud - self.u_ref.to(X.device, torch.float64)
        stage = torch.einsum("pti,ij,ptj->p", ex, self.Q_tor.to(X.device), ex) + torch.einsum("ti,ij,tj->", eu, self.R_tor.to(X.device), eu)
        if feedback:                                                      # each particle's own inputs
            eu = mc["inputs"][0] - self.u_ref.to(X.device, torch.float64)
            stage = torch.einsum("pti,ij,ptj->p", ex, self.Q_tor.to(X.device), ex) + torch.einsum("pti,ij,ptj->p", eu, self.R_tor.to(X.device), eu)
            Kh = Kfb if Kfb.dim() == 3 else Kfb[None].expand(H, da, ds)
            out["mean_lf"], out["cov_lf"] = lf["means"][0].cpu().numpy(), lf["covs"][0].cpu().numpy()
            out["input_cov_lf"] = torch.einsum("tik,tkl,tjl->tij", Kh, lf["covs"][0, :H], Kh).cpu().numpy()
            out["input_mean_mc"], out["input_cov_mc"] = mc["input_mean"][0].cpu().numpy(), mc["input_cov"][0].cpu().numpy()
            if self.input_constraints is not None:
                out["input_satisfaction"] = 1.0 - mc["input_violation"][0].cpu().numpy()
                out["input_requested"] = np.array([NormalDist().cdf(float(k)) for k in self.input_constraints.kappa])
                out["joint_input_satisfaction"] = 1.0 - float(mc["joint_input_violation"][0].item())
        out["stage_cost"] = float(stage.mean().item())
        if sc is not None:
            out["satisfaction"] = 1.0 - mc["violation"][0, 1:].cpu().numpy()
            out["requested"] = np.array([NormalDist().cdf(float(k)) for k in sc.kappa])
            out["joint_satisfaction"] = 1.0 - float(mc["joint_violation"][0].item())
        if P <= 4096:                                                     # (GPMPC_PARTICLE_COST_MAX_P: the particle cost sorts a row in LDS)
            from .particles import particle_cost
            pc = particle_cost(X.permute(1, 0, 2)[:, None].contiguous(), U[None], self._cost_params(), constraints=sc)
            out["cost_mc"], out["stage_mc"] = float(pc["cost"][0].item()), pc["stage"][0].cpu().numpy()
            if sc is not None:
                out["g_mc"] = pc["g"][0].cpu().numpy()
        return out

    # -- solve (src/mpc.py:269-330)
    def get_optimal_trajectory(self, curr_state, n_starts=None, solver=None):
        solver = getattr(self, "solver", None) if solver is None else solver
        if solver not in (None, "mppi", "lbfgs", "auglag"):
            raise ValueError("solver must be None, 'mppi', 'lbfgs' or 'auglag', got %r" % (solver,))
        lin = self._linearised()
        mmf = self._mm_full()
        if self._particles():
            if solver != "mppi":
                self._particles_refuse("solver=%r" % (solver,))
            if not 1 <= int(self.particle_options.get("particles", 256)) <= 4096:
                raise ValueError("particle_options['particles'] must be in 1..4096, got %r" % (self.particle_options.get("particles"),))
        if lin and solver in ("lbfgs", "auglag"):
            raise NotImplementedError("propagation='linearised' with solver=%r: the device L-BFGS and augmented-Lagrangian solvers run the "
                                      "moment-matched rollout (not yet); use solver=None, n_starts > 1 or solver='mppi'" % (solver,))
        if solver == "auglag":
            if getattr(self, "state_constraints", None) is None:
                raise ValueError("solver='auglag' is the constrained multi-start: without state constraints use solver='lbfgs'")
            if self.full_covariance and not mmf:
                raise NotImplementedError("solver='auglag' runs the diagonal rollout (gpmpc_auglag_solve): state constraints under the "
                                          "full-covariance rollout are not implemented")
        if solver == "lbfgs":
            if getattr(self, "state_constraints", None) is not None:
                raise NotImplementedError("solver='lbfgs' is unconstrained: state constraints under the device multi-start search (an "
                                          "augmented Lagrangian over the batched evaluation) are not implemented")
            if self.full_covariance and not mmf:
                raise NotImplementedError("solver='lbfgs' runs the diagonal rollout (gpmpc_lbfgs_solve): the search over the full-covariance "
                                          "rollout is not implemented")
        if solver == "mppi":
            if (self.n_starts if n_starts is None else n_starts) > 1:
                raise ValueError("solver='mppi' is one search over its own samples: it does not combine with n_starts > 1")
            if self._fullcov_mm():
                raise NotImplementedError("solver='mppi' runs the diagonal rollout (gpmpc_mppi_solve): MPPI over the full-covariance "
                                          "rollout is not implemented")
        k = getattr(self, "step_index", 0)
        self.step_index = k + 1
        if getattr(self, "reference", None) is not None:                   # the sliding window of this step, written into the one schedule before the solve
            r = self.reference(k)
            self.set_reference_trajectory(*(r if isinstance(r, tuple) else (r,)))
        if self.train_empty:
            if self.dynamics.gpr_err[0].num_train > 0:
                self.train_empty = False
            else:
                return np.zeros((self.horizon, self.input_dim))
        self.curr_state = torch.tensor(np.asarray(curr_state), device=self.device).type(torch.float64)
        self._cache_key = None
        x0 = np.zeros(shape=len(self.last_traj))          # warm start deliberately off, src/mpc.py:292-293
        lb, ub = self.horizon * list(self.lb), self.horizon * list(self.ub)
        K = self.n_starts if n_starts is None else n_starts
        sc = self.state_constraints
        if solver == "mppi":
            return self._keep_plan(self._solve_mppi())
        if solver == "auglag":
            return self._keep_plan(self._solve_device_auglag(max(int(K), 1), lb, ub))
        if solver == "lbfgs":
            return self._keep_plan(self._solve_device_lbfgs(max(int(K), 1), lb, ub))
        if sc is not None and self._fullcov_mm():
            raise NotImplementedError("state constraints under the full-covariance rollout are not implemented "
                                      "(q = a^T Sigma_t a and that path's Jacobian layout: a follow-up)")
        if sc is not None and K > 1 and mmf:
            raise NotImplementedError("propagation='moment_matching_full': the host lock-step multi-start solve is unconstrained -- use "
                                      "n_starts = 1, or solver='auglag' for a constrained multi-start on the full-covariance rule")
        if (sc is not None or self.input_constraints is not None) and K > 1:
            raise NotImplementedError("the lock-step multi-start solve is unconstrained: use n_starts = 1 with state constraints "
                                      "(a constrained multi-start, e.g. an augmented Lagrangian over the batched evaluation, is a follow-up)")
        if K > 1:
            return self._keep_plan(self._solve_multistart(K, lb, ub))
        if HAVE_CYIPOPT:
            if sc is None and self.input_constraints is None:
                nlp = cyipopt.Problem(n=len(x0), m=0, problem_obj=self, lb=lb, ub=ub, cl=[0], cu=[0])
            else:
                m = self.horizon * sum(self._rows())     # g <= 0: cl = -2e19 is Ipopt's "no lower bound"
                nlp = cyipopt.Problem(n=len(x0), m=m, problem_obj=self, lb=lb, ub=ub, cl=[-2e19] * m, cu=[0] * m)
            for k, v in (("mu_strategy", "adaptive"), ("accept_every_trial_step", "yes"), ("max_iter", 300),
                         ("tol", 1e-4), ("acceptable_tol", 1e-4), ("constr_viol_tol", 1e-4), ("compl_inf_tol", 1e-4),
                         ("dual_inf_tol", 1e-4), ("mu_target", 1e-4), ("acceptable_iter", 3), ("sb", "yes"),
                         ("print_level", 0)):
                nlp.add_option(k, v)
            x, _ = nlp.solve(x0)
            self.solver_used = "ipopt"
        else:
            x = self._solve_without_ipopt(x0, lb, ub)
        return self._keep_plan(x)

    def _keep_plan(self, x):
        """The end of every solve: the flat plan is kept for the next warm start and returned as (H, da)."""
        self.last_traj = x
        return np.reshape(x, (self.horizon, self.input_dim))

    def _starts(self, K, lb, ub, opt):
        """The K start points (K, H da) of a multi-start solve (multistart.make_starts): with ``opt["warm"]`` and a previous plan, that plan
        shifted by one step with its last input repeated; drawn from default_rng([opt["seed"], solve count]), and the solve is counted."""
        from .multistart import make_starts
        H, da = self.horizon, self.input_dim
        warm = None
        if opt.get("warm", True) and self.solver_used is not None:
            prev = np.asarray(self.last_traj, dtype=np.float64).reshape(H, da)
            warm = np.concatenate((prev[1:], prev[-1:]), axis=0).reshape(-1)
        rng = np.random.default_rng([int(opt.get("seed", 0)), self._solve_count])
        self._solve_count += 1
        return make_starts(K, H * da, lb, ub, rng, warm=warm, spread=float(opt.get("spread", 1.0)))

    def _solve_without_ipopt(self, x0, lb, ub):
        """Stand-in driver when cyipopt is not installed: bounded L-BFGS (scipy) on the same
        objective/gradient callbacks.  Not Ipopt: optimiser results are not parity-pinned."""
        from scipy.optimize import minimize
        big = 1e15
        bounds = [(None if l <= -big else l, None if u >= big else u) for l, u in zip(lb, ub)]
        if self.state_constraints is not None or self.input_constraints is not None:
            # SLSQP wants c(x) >= 0: c = -g.  Same callbacks as Ipopt would use; objective, gradient, g and its Jacobian on one x are
            # one device pass (the cache of _evaluate)
            m_c, n = sum(self._rows()), len(x0)
            cons = {"type": "ineq", "fun": lambda v: -np.asarray(self.constraints(v)),
                    "jac": lambda v: -np.asarray(self.jacobian(v)).reshape(self.horizon * m_c, n)}
            res = minimize(lambda v: self.objective(v), x0, jac=lambda v: np.asarray(self.gradient(v)).reshape(-1),
                           method="SLSQP", bounds=bounds, constraints=[cons], options={"maxiter": 300, "ftol": 1e-10})
            self.solver_used = "scipy-slsqp"
            self.last_solve_info = {"success": bool(res.success), "max_violation": float(np.max(self.constraints(res.x))),
                                    "iterations": int(res.nit), "message": str(res.message)}
            return res.x
        res = minimize(lambda v: self.objective(v), x0, jac=lambda v: np.asarray(self.gradient(v)).reshape(-1),
                       method="L-BFGS-B", bounds=bounds, options={"maxiter": 300, "ftol": 1e-10, "gtol": 1e-4})
        self.solver_used = "scipy-lbfgsb"
        return res.x

    def _solve_mppi(self):
        """The sampling planner (mppi.mppi_solve) from the previous plan shifted by one step (zeros on the first solve); the call index of
        the noise is the solve count (shared with the multi-start's start sampler), so a loop of solves is reproducible from ``mppi_options["seed"]``."""
        from .mppi import mppi_solve
        from .linearised import mppi_solve_linearised
        opt = self.mppi_options
        H, da = self.horizon, self.input_dim
        big = 1e15                                                        # (the setters' "no bound", as _solve_without_ipopt reads it)
        lb = np.array([-np.inf if v <= -big else v for v in self.lb], dtype=np.float64)
        ub = np.array([np.inf if v >= big else v for v in self.ub], dtype=np.float64)
        sigma = opt.get("sigma")
        if sigma is None:
            sigma = np.where(np.isfinite(ub - lb), 0.25 * (ub - lb), 1.0)
        start = np.zeros((H, da))
        if self.solver_used is not None:                                  # (whichever solver made the previous plan)
            prev = np.asarray(self.last_traj, dtype=np.float64).reshape(H, da)
            start = np.clip(np.concatenate((prev[1:], prev[-1:]), axis=0), lb, ub)
        lin = self._linearised()
        if self._particles():
            from .particles import mppi_solve_particles
            pk = self._particle_kw()
            r = mppi_solve_particles(self._linearised_model(self.dynamics.pack()), self.curr_state, start, self._cost_params(),
                                     constraints=self.state_constraints, particles=pk["particles"], samples=int(opt.get("samples", 64)),
                                     iterations=int(opt.get("iterations", 30)), sigma=sigma, decay=float(opt.get("decay", 0.9)),
                                     beta=float(opt.get("beta", 0.1)), seed=pk["seed"], call_index=pk["call_index"], lb=lb, ub=ub)
            return self._mppi_done(r, opt, "mppi-particles x%d P%d" % (int(opt.get("samples", 64)), pk["particles"]))
        solve = mppi_solve_linearised if lin else mppi_solve
        r = solve(self._linearised_model(self.dynamics.pack()) if lin else self.dynamics.pack(), self.curr_state, start, self._cost_params(),
                  constraints=self.state_constraints, samples=int(opt.get("samples", 64)), iterations=int(opt.get("iterations", 30)), sigma=sigma,
                  decay=float(opt.get("decay", 0.9)), beta=float(opt.get("beta", 0.1)), seed=int(opt.get("seed", 0)),
                  call_index=self._solve_count, lb=lb, ub=ub,
                  **(dict(self._lin_kw(), form=self.linearised_form) if lin else ({"full_covariance": True} if self._mm_full() else {})))
        return self._mppi_done(r, opt, "mppi x%d" % int(opt.get("samples", 64)))

    def _mppi_done(self, r, opt, used):
        """The end of an MPPI solve under every propagation: the solve is counted and its result kept."""
        self._solve_count += 1
        self.solver_used = used
        self.last_solve_info = {"cost": r["cost"], "violation": r["violation"], "feasible": r["feasible"], "success": r["feasible"],
                                "max_violation": r["violation"], "iterations": int(opt.get("iterations", 30)), "trace": r["trace"]}
        self._cache_key = None
        return r["U"].reshape(-1)

    def _solve_device_lbfgs(self, K, lb, ub):
        """The lock-step multi-start search on the device (device_lbfgs.lbfgs_solve): the starts, the seed and the solve count are those of
        ``_solve_multistart``; the ticks run as enqueues of ``check_every`` (rollout, tick kernel) pairs without the host in between."""
        from .device_lbfgs import lbfgs_solve
        opt = self.multistart_options
        H, da = self.horizon, self.input_dim
        X0 = self._starts(K, lb, ub, opt)
        U, cost, info = lbfgs_solve(self.dynamics.pack(), self.curr_state, X0.reshape(K, H, da), self._cost_params(),
                                    lb=np.asarray(self.lb, dtype=np.float64), ub=np.asarray(self.ub, dtype=np.float64),
                                    max_ticks=int(opt.get("max_ticks", 150)), history=int(opt.get("history", 8)),
                                    gtol=float(opt.get("gtol", 1e-4)), ftol=float(opt.get("ftol", 1e-10)),
                                    check_every=int(opt.get("check_every", 8)), full_covariance=self._mm_full())
        info["starts"] = K
        info["sharded_over"] = 1
        self.last_solve_info = info
        self.solver_used = f"device-lbfgs x{K}"
        self._cache_key = None
        return U.reshape(-1)

    def _solve_device_auglag(self, K, lb, ub):
        """The constrained multi-start on the device (device_auglag.auglag_solve): the starts, the seed and the solve count are those of
        ``_solve_device_lbfgs`` (``spread``, ``seed``, ``warm`` from ``multistart_options``); everything else from ``auglag_options``."""
        from .device_auglag import auglag_solve
        H, da = self.horizon, self.input_dim
        X0 = self._starts(K, lb, ub, self.multistart_options)
        U, cost, info = auglag_solve(self.dynamics.pack(), self.curr_state, X0.reshape(K, H, da), self._cost_params(), self.state_constraints,
                                     lb=np.asarray(self.lb, dtype=np.float64), ub=np.asarray(self.ub, dtype=np.float64),
                                     full_covariance=self._mm_full(), **self.auglag_options)
        best = info["best"]
        info["starts"] = K
        info["success"] = bool(info["feasible"][best])
        info["max_violation"] = float(info["violation"][best])
        self.last_solve_info = info
        self.solver_used = f"device-auglag x{K}"
        self._cache_key = None
        return U.reshape(-1)

    def _solve_multistart(self, K, lb, ub):
        """K starts advanced together (multistart.lockstep_lbfgs): one batched rollout of K plans per solver iteration, replayed as
        one hipGraph; with torch.distributed initialised the K plans are sharded over the ranks (parallel.sharded_rollout) and every
        rank takes the same decisions from the same gathered [cost | grad].  Optimiser results unpinned, like the Ipopt stand-in."""
        from .multistart import lockstep_lbfgs
        opt = self.multistart_options
        n, H, da = self.horizon * self.input_dim, self.horizon, self.input_dim
        pack, cp, cs = self.dynamics.pack(), self._cost_params(), self.curr_state
        X0 = self._starts(K, lb, ub, opt)
        dist = None
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            dist = torch.distributed

        lin = self._linearised()
        mmf = self._mm_full()

        def run(x0b, Ub, graph):
            if lin:                                                       # (plain launches: graph replay of the linearised rollout is not provided)
                from .linearised import linearised_rollout
                return linearised_rollout(self._linearised_model(pack), x0b, Ub, cp, want_grad=True, want_traj=False, form=self.linearised_form,
                                          **self._lin_kw())
            if self.full_covariance or mmf:
                return rollout_fullcov(pack, x0b, Ub, cp, want_grad=True)
            return rollout(pack, x0b, Ub, cp, want_grad=True, want_traj=False, graph=graph)

        def evaluate(X):                                                  # (K, n), or (S K, n): S step lengths per start
            nb = X.shape[0]
            U = np.ascontiguousarray(X.reshape(nb, H, da))
            if dist is not None:
                from .parallel import sharded_rollout
                Ud = torch.as_tensor(U, device=self.device)
                c, g = sharded_rollout(lambda x0b, Ub: run(x0b, Ub, False), cs, Ud, dist)
                return c.cpu().numpy(), g.cpu().numpy().reshape(nb, n)
            r = run(cs, U, True)
            if "cost_grad" in r:                                          # cost and gradient in ONE device-to-host copy
                cg = r["cost_grad"].cpu().numpy()
                return cg[:nb], cg[nb:].reshape(nb, n)
            return r["cost"].cpu().numpy(), r["grad"].cpu().numpy().reshape(nb, n)

        x, info = lockstep_lbfgs(evaluate, X0, np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64),
                                 max_ticks=int(opt.get("max_ticks", 150)), history=int(opt.get("history", 8)),
                                 gtol=float(opt.get("gtol", 1e-4)), ftol=float(opt.get("ftol", 1e-10)), patience=opt.get("patience"),
                                 line_points=int(opt.get("line_points", 1)))
        info["starts"] = K
        info["sharded_over"] = dist.get_world_size() if dist is not None else 1
        self.last_solve_info = info
        self.solver_used = f"lockstep-lbfgs x{K}"
        self._cache_key = None
        return x
