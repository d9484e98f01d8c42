"""Thin, batched host API over the C ABI: GP pack, cost parameters, rollout, moment matching.

Everything here is plumbing (device buffers, streams, argument marshalling); the
arithmetic lives in csrc/*.hip.  Tensors are float64 CUDA tensors; numpy inputs are
copied to the current device.
"""
import ctypes
import functools

import numpy as np
import torch

from . import _lib
from ._lib import CostParamsC, InputConstraintsC, StateConstraintsC, check, lib, ptr, require_gpu, stream_ptr, host_doubles


def _dev(a, device):
    if isinstance(a, torch.Tensor):
        return a.detach().to(device=device, dtype=torch.float64).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64)), device=device)


def _empty(device, *shape):
    return torch.empty(shape, dtype=torch.float64, device=device)


def _problem(pack, x0, U, cost):
    """What every rollout does to its inputs: U (a device tensor, or the float64 host array of the graph path) to (B, H, da), x0 to a
    device tensor (B, ds) -- one start state serves all trajectories --, both checked against the pack and the cost.
    Returns (x0, U, B, H, da)."""
    if U.ndim == 2:
        U = U[None]
    B, H, da = U.shape
    x0 = _dev(x0, pack.device).reshape(-1, pack.ds)
    if x0.shape[0] == 1 and B > 1:
        x0 = x0.expand(B, pack.ds).contiguous()
    if da != pack.da or x0.shape[0] != B or cost.ds != pack.ds or cost.da != pack.da:
        raise ValueError("shape mismatch between pack, x0, U and cost parameters")
    return x0, U, B, H, da


def _describe(buf):
    """The ``key=value`` words of a ``*_describe`` entry as a dict (integers as int)."""
    out = {}
    for kv in buf.value.decode().split():
        k, v = kv.split("=", 1)
        out[k] = int(v) if v.lstrip("-").isdigit() else v
    return out


class CostSchedule:
    """Time-varying references and a terminal weight for every cost of the library (C ABI ``gpmpc_cost_schedule_*``; no reference
    counterpart: src/mpc.py holds one x_ref, one u_ref, one Q).  ONE device buffer for horizons up to ``H_max``, owned by the library and
    addressed by ``id``; its contents are read by the cost kernels from device memory, so a :meth:`set` between two graph replays takes
    effect without a new capture.  Hand it to ``CostParams(..., schedule=cs)``; ``x_ref`` / ``u_ref`` of those parameters are then ignored."""

    def __init__(self, H_max, ds, da, device=None):
        self.device = device if device is not None else require_gpu()
        self.H_max, self.ds, self.da = int(H_max), int(ds), int(da)
        self.H = 0
        self.has_Q_terminal = False
        self.id = 0
        out = ctypes.c_int(0)
        with torch.cuda.device(self.device):
            check(lib().gpmpc_cost_schedule_create(self.H_max, self.ds, self.da, ctypes.byref(out)), "gpmpc_cost_schedule_create")
        self.id = out.value

    def set(self, X_ref, U_ref=None, Q_terminal=None):
        """X_ref (H+1, ds), U_ref (H, da) or None = zeros, Q_terminal (ds, ds) or None = no terminal weight; H <= H_max.  Host arrays
        (checked for finiteness, consumed before the call returns), or CUDA float64 tensors on the schedule's device (copied in stream
        order without the host; all of them tensors then)."""
        dev_form = isinstance(X_ref, torch.Tensor) and X_ref.is_cuda
        shape = tuple(X_ref.shape)
        if len(shape) != 2 or shape[1] != self.ds or shape[0] < 2:
            raise ValueError("X_ref must be (H + 1, %d), got %s" % (self.ds, shape))
        H = shape[0] - 1
        if U_ref is not None and tuple(np.shape(U_ref)) != (H, self.da):
            raise ValueError("U_ref must be (%d, %d), got %s" % (H, self.da, tuple(np.shape(U_ref))))
        if Q_terminal is not None and tuple(np.shape(Q_terminal)) != (self.ds, self.ds):
            raise ValueError("Q_terminal must be (%d, %d), got %s" % (self.ds, self.ds, tuple(np.shape(Q_terminal))))
        with torch.cuda.device(self.device):
            if dev_form:
                t = [None if a is None else _dev(a, self.device) for a in (X_ref, U_ref, Q_terminal)]
                check(lib().gpmpc_cost_schedule_set_dev(self.id, H, ptr(t[0]), ptr(t[1]), ptr(t[2]), stream_ptr()), "gpmpc_cost_schedule_set_dev")
            else:
                h = [None if a is None else host_doubles(a) for a in (X_ref, U_ref, Q_terminal)]
                check(lib().gpmpc_cost_schedule_set(self.id, H, *[None if a is None else a[1] for a in h], stream_ptr()),
                      "gpmpc_cost_schedule_set")
        self.H, self.has_Q_terminal = H, Q_terminal is not None
        return self

    def get(self):
        """What the library holds: dict with H_max, ds, da, H, has_Q_terminal and the device pointer ``ptr`` (constant for the life of the id)."""
        v = [ctypes.c_int() for _ in range(5)]
        p = ctypes.c_void_p()
        check(lib().gpmpc_cost_schedule_get(self.id, *[ctypes.byref(x) for x in v], ctypes.byref(p)), "gpmpc_cost_schedule_get")
        return dict(H_max=v[0].value, ds=v[1].value, da=v[2].value, H=v[3].value, has_Q_terminal=bool(v[4].value), ptr=p.value)

    def close(self):
        """Destroy the schedule (the library waits for the device first).  Cost parameters that still name the id are refused afterwards."""
        if self.id:
            i, self.id = self.id, 0
            with torch.cuda.device(self.device):
                check(lib().gpmpc_cost_schedule_destroy(i), "gpmpc_cost_schedule_destroy")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CostParams:
    """Parameters of RiskSensitiveMPC.cost_torch (reference src/mpc.py:156-200).  schedule: a :class:`CostSchedule` whose rows replace
    ``x_ref`` / ``u_ref`` and whose terminal weight, where set, replaces ``Q`` at the last step."""

    def __init__(self, gamma, Q, R, R_delta=None, x_ref=None, u_ref=None, last_u=None, schedule=None):
        Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
        R = np.atleast_2d(np.asarray(R, dtype=np.float64))
        self.ds, self.da = Q.shape[0], R.shape[0]
        if Q.shape != (self.ds, self.ds) or R.shape != (self.da, self.da):
            raise ValueError("Q and R must be square")
        if self.ds > _lib.MAX_DS or self.da > _lib.MAX_D:
            raise ValueError("state / input dimension exceeds the library limits")
        c = CostParamsC()
        c.gamma = float(gamma)
        c.Q[:self.ds * self.ds] = Q.reshape(-1).tolist()
        c.R[:self.da * self.da] = R.reshape(-1).tolist()
        if R_delta is not None:
            Rd = np.atleast_2d(np.asarray(R_delta, dtype=np.float64))
            c.R_delta[:self.da * self.da] = Rd.reshape(-1).tolist()
            c.has_R_delta = 1
            lu = np.zeros(self.da) if last_u is None else np.asarray(last_u, dtype=np.float64).reshape(-1)[:self.da]
            c.last_u[:self.da] = lu.tolist()
        xr = np.zeros(self.ds) if x_ref is None else np.asarray(x_ref, dtype=np.float64).reshape(-1)
        ur = np.zeros(self.da) if u_ref is None else np.asarray(u_ref, dtype=np.float64).reshape(-1)
        c.x_ref[:self.ds] = xr.tolist()
        c.u_ref[:self.da] = ur.tolist()
        if schedule is not None:
            if (schedule.ds, schedule.da) != (self.ds, self.da):
                raise ValueError("the cost schedule has dimensions (%d, %d), the cost (%d, %d)" % (schedule.ds, schedule.da, self.ds, self.da))
            c.schedule_id = int(schedule.id)
        self.schedule = schedule             # (kept alive with the parameters that name it)
        self.c = c


class StateConstraints:
    """Linear chance constraints on the state, held at every horizon step t = 1..H (C ABI ``gpmpc_state_constraints``; no reference
    counterpart: src/mpc.py:257-267 returns 0):

        g[t, r] = A[r] . mu_t + kappa[r] * sqrt(sum_k A[r, k]^2 var_t[k]) - b[r]  <=  0

    A: (m_c, ds) or (ds,); b: (m_c,) or scalar.  Exactly one of ``kappa`` (>= 0) and ``prob`` (one-sided satisfaction probability in
    [0.5, 1), kappa = Phi^-1(prob)), each a scalar or one value per row; kappa = 0 (prob = 0.5) constrains the mean only.
    The rollout does not clamp negative variances: a non-positive variance sum counts as sd = 0 (the row is then its mean part, in value
    and derivative); NaN passes through to every row of that step."""

    def __init__(self, A, b, kappa=None, prob=None):
        if (kappa is None) == (prob is None):
            raise ValueError("give exactly one of kappa and prob")
        A = np.atleast_2d(np.asarray(A, dtype=np.float64))
        m, ds = A.shape
        if not 1 <= m <= _lib.MAX_CONS:
            raise ValueError(f"1 to {_lib.MAX_CONS} constraint rows are supported, got {m}")
        if not 1 <= ds <= _lib.MAX_DS:
            raise ValueError("state dimension exceeds the library limits")
        b = np.broadcast_to(np.asarray(b, dtype=np.float64).reshape(-1), (m,)).copy()
        if prob is not None:
            from statistics import NormalDist
            pr = np.broadcast_to(np.asarray(prob, dtype=np.float64).reshape(-1), (m,))
            if not np.all((pr >= 0.5) & (pr < 1.0)):
                raise ValueError("prob must lie in [0.5, 1): kappa = Phi^-1(prob) >= 0")
            kap = np.array([NormalDist().inv_cdf(float(v)) if v > 0.5 else 0.0 for v in pr])
        else:
            kap = np.broadcast_to(np.asarray(kappa, dtype=np.float64).reshape(-1), (m,)).copy()
            if not np.all(kap >= 0.0):                      # (NaN fails too)
                raise ValueError("kappa must be >= 0")
        if not (np.all(np.isfinite(A)) and np.all(np.isfinite(b)) and np.all(np.isfinite(kap))):
            raise ValueError("constraint rows must be finite")
        self.A, self.b, self.kappa = A, b, kap
        self.m, self.ds = m, ds
        c = StateConstraintsC()
        c.n_rows = m
        c.A[:m * ds] = A.reshape(-1).tolist()
        c.b[:m] = b.tolist()
        c.kappa[:m] = kap.tolist()
        self.c = c

    @classmethod
    def box(cls, lb, ub, state_dim, prob=None, kappa=None):
        """Rows x_k <= ub[k] and -x_k <= -lb[k] for every finite bound (``None`` and +-inf entries produce no row; ``lb`` / ``ub`` may
        themselves be None), upper bounds first, each group in state order."""
        rows, rhs = [], []
        for bound, sign in ((ub, 1.0), (lb, -1.0)):
            if bound is None:
                continue
            bound = list(bound)
            if len(bound) != state_dim:
                raise ValueError("one bound (or None) per state dimension")
            for k, v in enumerate(bound):
                if v is None or not np.isfinite(v):
                    continue
                a = np.zeros(state_dim)
                a[k] = sign
                rows.append(a)
                rhs.append(sign * float(v))
        if not rows:
            raise ValueError("no finite bound given")
        return cls(np.array(rows), np.array(rhs), kappa=kappa, prob=prob)


class InputConstraints:
    """Linear chance constraints on the COMMANDED input u_t = v_t + K_t (x_t - mu_t) of the full-covariance linearised rollout, held at
    every step t = 0..H-1 (C ABI ``gpmpc_input_constraints``):

        g_u[t, r] = C[r] . v_t + kappa[r] * sqrt(a^T Sigma_t a) - d[r]  <=  0,      a = K_t^T C[r]

    C: (m_u, da) or (da,); d: (m_u,) or scalar; ``kappa`` / ``prob`` as ``StateConstraints``.  Without a gain the rows bound v_t alone."""

    def __init__(self, C, d, kappa=None, prob=None):
        s = StateConstraints(C, d, kappa=kappa, prob=prob)                   # the same checks: rows, finiteness, kappa >= 0
        self.C, self.d, self.kappa = s.A, s.b, s.kappa
        self.m, self.da = s.m, s.ds
        c = InputConstraintsC()
        c.n_rows = self.m
        c.C[:self.m * self.da] = self.C.reshape(-1).tolist()
        c.d[:self.m] = self.d.tolist()
        c.kappa[:self.m] = self.kappa.tolist()
        self.c = c

    @classmethod
    def box(cls, lb, ub, da, prob=None, kappa=None):
        """Rows u_j <= ub[j] and -u_j <= -lb[j] for every finite bound, as ``StateConstraints.box``."""
        s = StateConstraints.box(lb, ub, da, prob=prob, kappa=kappa)
        return cls(s.A, s.b, kappa=s.kappa)


def noise_arrays(ds, da, init_cov=None, action_var=None, process_var=None):
    """The three parts of a noise model as contiguous float64 arrays of the pack's shapes (None stays None): shapes are checked here, values
    by the library."""
    P = av = pv = None
    if init_cov is not None:
        P = np.asarray(init_cov, dtype=np.float64)
        if P.ndim == 0:
            P = np.full(ds, float(P))
        if P.ndim == 1:
            if P.shape[0] != ds:
                raise ValueError(f"init_cov: a vector of {ds} variances or a ({ds}, {ds}) matrix, got shape {P.shape}")
            P = np.diag(P)
        if P.shape != (ds, ds):
            raise ValueError(f"init_cov: a vector of {ds} variances or a ({ds}, {ds}) matrix, got shape {P.shape}")
        P = np.ascontiguousarray(P)
    if action_var is not None:
        av = np.asarray(action_var, dtype=np.float64)
        if av.ndim > 1 or (av.ndim == 1 and av.shape[0] != da):
            raise ValueError(f"action_var: {da} variances, got shape {av.shape}")
        av = np.ascontiguousarray(np.broadcast_to(av, (da,)))
        if da == 0:
            av = None
    if process_var is not None:
        pv = np.asarray(process_var, dtype=np.float64)
        if pv.ndim > 1 or (pv.ndim == 1 and pv.shape[0] != ds):
            raise ValueError(f"process_var: {ds} variances, got shape {pv.shape}")
        pv = np.ascontiguousarray(np.broadcast_to(pv, (ds,)))
    return P, av, pv


class GPPack:
    """Device-resident state of ``ds`` GPs sharing X (reference: what Dynamics +
    GaussianProcessRegression hold, src/dynamics.py:33-37, src/gpr.py:24-36) folded into
    the per-data-update constants of the rollout (beta, weight matrices)."""

    def __init__(self, X, Y, Ky_inv, lambdas, sigma_f, device=None, y_is_beta=False, nominal=None, fullcov=False):
        """Y: (N, ds) targets, or the beta vectors themselves when ``y_is_beta`` (then Ky_inv may be
        None: only means and cross-covariances are meaningful).
        nominal: (W (ds, D), b (ds,) or scalar) of a linear nominal model m_a(z) = W[a] . z + b[a], z = (x, u): Y stays the RAW targets, the
        library forms beta from Y - X W^T - b and the rollout adds the model back exactly (with ``y_is_beta`` beta is taken as given).
        fullcov: the cross-covariance weights exist from creation on (``enable_fullcov`` BEFORE the first build, which then fills them)."""
        self.device = device if device is not None else require_gpu()
        self._h = None
        self.generation = 0          # bumped by every (re)build: caches keyed on the pack object include it
        self._drop_caches()
        self.fullcov = False
        self._nominal = None
        self._fill(X, Y, Ky_inv, lambdas, sigma_f, y_is_beta, nominal, fullcov)

    def _drop_caches(self):
        """Forget the per-stream workspaces and the buffers of the graph path: the plans they were sized for are gone."""
        self._graph_bufs = {}
        self._ws = {}

    def _set_nominal(self, nominal):
        """Hand a changed model to the library (switching it on or off re-plans the pack: scratch sizes change)."""
        if nominal is not None:
            W = np.ascontiguousarray(np.asarray(nominal[0], dtype=np.float64).reshape(self.ds, self.D))
            b = np.ascontiguousarray(np.broadcast_to(np.asarray(nominal[1], dtype=np.float64).reshape(-1), (self.ds,)))
            if not (np.all(np.isfinite(W)) and np.all(np.isfinite(b))):
                raise ValueError("nominal model coefficients must be finite")
            nominal = (W, b)
        old = self.nominal                               # (as the LIBRARY holds it: the handle may have been given another model directly)
        if (nominal is None and old is None) or (nominal is not None and old is not None and np.array_equal(nominal[0], old[0])
                                                 and np.array_equal(nominal[1], old[1])):
            return
        with torch.cuda.device(self.device):
            if nominal is None:
                check(lib().gpmpc_pack_set_nominal(self._h, None, None, stream_ptr()), "gpmpc_pack_set_nominal")
            else:
                check(lib().gpmpc_pack_set_nominal(self._h, host_doubles(nominal[0])[1], host_doubles(nominal[1])[1], stream_ptr()),
                      "gpmpc_pack_set_nominal")
        if (nominal is None) != (old is None):
            self._drop_caches()
        self._nominal = nominal

    @property
    def nominal(self):
        """(W (ds, D), b (ds,)) of the pack's linear nominal model as the library holds it, or None."""
        if self._h is None:
            return None
        W, b = np.zeros((self.ds, self.D)), np.zeros(self.ds)
        rc = lib().gpmpc_pack_get_nominal(self._h, host_doubles(W)[1], host_doubles(b)[1])
        if rc < 0:
            check(rc, "gpmpc_pack_get_nominal")
        return (W, b) if rc == 1 else None

    def set_noise(self, init_cov=None, action_var=None, process_var=None):
        """Noise model of the rollout (C ABI ``gpmpc_pack_set_noise``), shared by all trajectories of a call.
        init_cov: covariance of the start state, (ds, ds) symmetric or a (ds,) vector taken as a diagonal (a scalar: that value on the
        diagonal); the diagonal rollout uses its diagonal, ``rollout_fullcov`` the whole matrix.  action_var: (da,) variance of each input at
        every step (a scalar is broadcast).  process_var: (ds,) added to the predicted variance of each state at every step t >= 1.
        None resets a part to its default (1e-3 I, float32(1e-3), 0); all None restores the defaults.  The values are read from device
        memory by the kernels: no captured graph, plan or buffer of the pack is dropped."""
        if isinstance(process_var, str):
            raise ValueError('process_var="sigma_n" is understood by Dynamics.set_noise_model: a pack does not know the noise of its GPs')
        P, av, pv = noise_arrays(self.ds, self.da, init_cov, action_var, process_var)
        hp = lambda a: None if a is None else host_doubles(a)[1]  # noqa: E731
        with torch.cuda.device(self.device):
            check(lib().gpmpc_pack_set_noise(self._h, hp(P), hp(av), hp(pv), stream_ptr()), "gpmpc_pack_set_noise")
        return self

    @property
    def noise(self):
        """(init_cov (ds, ds), action_var (da,), process_var (ds,)) as the library holds them."""
        P, av, pv = np.zeros((self.ds, self.ds)), np.zeros(max(self.da, 1)), np.zeros(self.ds)
        rc = lib().gpmpc_pack_get_noise(self._h, host_doubles(P)[1], host_doubles(av)[1], host_doubles(pv)[1])
        if rc < 0:
            check(rc, "gpmpc_pack_get_noise")
        return P, av[:self.da], pv

    @property
    def noise_is_default(self):
        return lib().gpmpc_pack_get_noise(self._h, None, None, None) == 0

    def _fill(self, X, Y, Ky_inv, lambdas, sigma_f, y_is_beta, nominal=None, fullcov_first=False):
        self.X = _dev(X, self.device)
        Y = _dev(Y, self.device)
        self.Y = Y.reshape(self.X.shape[0], -1)
        self.N, self.D = self.X.shape
        self.ds = self.Y.shape[1]
        self.da = self.D - self.ds
        ld = gstride = 0
        if Ky_inv is not None:
            Kt = Ky_inv if isinstance(Ky_inv, torch.Tensor) else None
            if (Kt is not None and Kt.is_cuda and Kt.device == self.device and Kt.dtype == torch.float64 and not Kt.is_contiguous()
                    and Kt.stride(-1) == 1 and Kt.shape[-2:] == (self.N, self.N) and (Kt.dim() == 2 or (Kt.dim() == 3 and Kt.shape[0] == self.ds))):
                # a view of a capacity-padded buffer (closed loop) and / or ONE matrix shared by all GPs: read in place
                ld, gstride = Kt.stride(-2), (0 if Kt.dim() == 2 else Kt.stride(0))
                Ky_inv = Kt
            elif Kt is not None and Kt.dim() == 2 and self.ds > 1 and tuple(Kt.shape) == (self.N, self.N):
                Ky_inv = _dev(Kt, self.device)          # one contiguous matrix shared by all GPs
                ld, gstride = self.N, 0
            else:
                Ky_inv = _dev(Ky_inv, self.device).reshape(self.ds, self.N, self.N)
        self.lambdas = np.ascontiguousarray(np.asarray(lambdas, dtype=np.float64).reshape(self.ds, self.D))
        self.sigma_f = np.ascontiguousarray(np.asarray(sigma_f, dtype=np.float64).reshape(self.ds))
        if self._h is None:
            h = ctypes.c_void_p()
            with torch.cuda.device(self.device):       # the pack's HBM buffers belong to THIS device, whatever is current
                check(lib().gpmpc_pack_create(ctypes.byref(h), self.N, self.ds, self.da), "gpmpc_pack_create")
            self._h = h
            if fullcov_first:
                self.enable_fullcov()
        self._set_nominal(nominal)
        _, lp = host_doubles(self.lambdas)
        _, sp = host_doubles(self.sigma_f)
        with torch.cuda.device(self.device):
            if ld and not y_is_beta:
                check(lib().gpmpc_pack_build_strided(self._h, ptr(self.X), ptr(self.Y), ctypes.c_void_p(Ky_inv.data_ptr()), ld, gstride,
                                                     lp, sp, stream_ptr()), "gpmpc_pack_build_strided")
            else:
                if ld:                                  # (beta given: the strided entry takes targets only)
                    Ky_inv = Ky_inv.contiguous() if Ky_inv.dim() == 3 else Ky_inv.contiguous().unsqueeze(0).expand(self.ds, -1, -1).contiguous()
                build = lib().gpmpc_pack_build_beta if y_is_beta else lib().gpmpc_pack_build
                check(build(self._h, ptr(self.X), ptr(self.Y), ptr(Ky_inv), lp, sp, stream_ptr()), "gpmpc_pack_build")
        n, npad, ds, da = (ctypes.c_int() for _ in range(4))
        lib().gpmpc_pack_dims(self._h, ctypes.byref(n), ctypes.byref(npad), ctypes.byref(ds), ctypes.byref(da))
        self.Np = npad.value
        self.generation += 1

    def rebuild(self, X, Y, Ky_inv, lambdas, sigma_f, nominal="keep", y_is_beta=False):
        """Refill THIS pack for new data / hyper-parameters when its allocation fits (same device, dimensions and padded
        size): no allocation, the library handle survives.  Returns False (pack untouched) when it does not fit.
        nominal: as in the constructor; None clears the model, the default keeps the one the pack has.
        y_is_beta: as in the constructor (a sparse GP refills its pack with (Z, alpha, Q) after every data update)."""
        Xs = X.shape
        n, D = int(Xs[0]), int(Xs[1])
        ds = int(Y.shape[1]) if len(Y.shape) > 1 else 1
        if self._h is None or D != self.D or ds != self.ds or ((n + 63) // 64) * 64 != self.Np:
            return False
        with torch.cuda.device(self.device):
            if n != self.N:
                check(lib().gpmpc_pack_resize(self._h, n), "gpmpc_pack_resize")
        self._fill(X, Y, Ky_inv, lambdas, sigma_f, bool(y_is_beta),      # (cross-covariance weights, if enabled, follow every build)
                   self._nominal if isinstance(nominal, str) and nominal == "keep" else nominal)
        return True

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                torch.cuda.synchronize(self.device)
                with torch.cuda.device(self.device):
                    lib().gpmpc_pack_destroy(h)
            except Exception:
                pass
            self._h = None

    def enable_fullcov(self):
        """Allocate the cross-covariance weight matrices (one N x N per GP pair): full-covariance rollout and
        analytic cross-covariance Jacobians."""
        with torch.cuda.device(self.device):
            check(lib().gpmpc_pack_enable_fullcov(self._h, stream_ptr()), "gpmpc_pack_enable_fullcov")
        self.fullcov = True
        return self

    def objective_gradient(self, x0_host, U_host, cost, want_grad=True):
        """One solver callback (C ABI ``gpmpc_objective_gradient``; reference src/mpc.py:202-255): host arrays in, host
        array out.  x0_host (ds,), U_host (H, da) float64 numpy -> numpy [cost, d cost / d U (H*da)].  Synchronous."""
        x0 = np.ascontiguousarray(x0_host, dtype=np.float64).reshape(-1)
        U = np.ascontiguousarray(U_host, dtype=np.float64).reshape(-1, self.da)
        if x0.shape[0] != self.ds or cost.ds != self.ds or cost.da != self.da:
            raise ValueError("shape mismatch between pack, x0, U and cost parameters")
        H = U.shape[0]
        out = np.empty(1 + (H * self.da if want_grad else 0), dtype=np.float64)
        dp = ctypes.POINTER(ctypes.c_double)
        with torch.cuda.device(self.device):
            check(lib().gpmpc_objective_gradient(self._h, H, x0.ctypes.data_as(dp), U.ctypes.data_as(dp), ctypes.byref(cost.c),
                                                 _lib.WANT_GRAD if want_grad else 0, out.ctypes.data_as(dp), stream_ptr(self.device)),
                  "gpmpc_objective_gradient")
        return out

    def reload_tuning(self):
        """Re-read the GPMPC_* tuning environment variables (read once at pack creation otherwise)."""
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            check(lib().gpmpc_pack_reload_tuning(self._h), "gpmpc_pack_reload_tuning")
        self._drop_caches()
        return self

    def plan(self, B, H, want_grad=True, graph=False):
        """What a rollout call of this shape launches (C ABI ``gpmpc_plan_describe``): dict with ``form``, ``kernel``, ``tiling``,
        ``workgroups`` (per horizon step), ``launches_per_step``, ``split`` ..."""
        buf = ctypes.create_string_buffer(512)
        flags = (_lib.WANT_GRAD if want_grad else 0) | (_lib.USE_GRAPH if graph else 0)
        check(lib().gpmpc_plan_describe(self._h, int(B), int(H), flags, buf, 512), "gpmpc_plan_describe")
        return _describe(buf)

    def plan_fullcov(self, B, H, want_grad=True):
        """What ``rollout_fullcov`` launches for this call shape (C ABI ``gpmpc_rollout_fullcov_describe``): dict with ``form``
        (``two_launch`` | ``four_launch``), ``tiling``, ``workgroups``, ``columns_per_iteration``, ``head_workgroups_per_unit``, ``kernel``."""
        buf = ctypes.create_string_buffer(512)
        check(lib().gpmpc_rollout_fullcov_describe(self._h, int(B), int(H), _lib.WANT_GRAD if want_grad else 0, buf, 512),
              "gpmpc_rollout_fullcov_describe")
        return _describe(buf)

    def plan_moment_match(self, nq, want_cov=False, want_grad=False, bug_compatible=False):
        """What ``moment_match`` launches for nq queries with these options (C ABI ``gpmpc_moment_match_describe``; nothing runs):
        dict with ``tiling``, ``sbf`` (1: scalar-broadcast pair kernel), ``tb``, ``waves``, ``nunits``, ``nwork``, ``cross``
        (``pair`` | ``direct`` | ``none``: who evaluates the cross-covariances and their Jacobians) and ``workspace`` (bytes this call needs)."""
        buf = ctypes.create_string_buffer(256)
        flags = ((_lib.WANT_GRAD if want_grad else 0) | (_lib.COV_BUG_COMPAT if bug_compatible else 0)
                 | (_lib.DESCRIBE_WANT_COV if want_cov else 0))
        check(lib().gpmpc_moment_match_describe(self._h, int(nq), flags, buf, 256), "gpmpc_moment_match_describe")
        return _describe(buf)

    def autotune(self, B, H, want_grad=True, graph=False):
        """Time the candidate plans of this call shape on this device and keep the fastest for later calls (C ABI
        ``gpmpc_pack_autotune``).  Returns a list of dicts (``name``, ``ms``, ``winner``, plan fields), the default plan first."""
        buf = ctypes.create_string_buffer(8192)
        flags = (_lib.WANT_GRAD if want_grad else 0) | (_lib.USE_GRAPH if graph else 0)
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            rc = lib().gpmpc_pack_autotune(self._h, int(B), int(H), flags, buf, 8192)
        if rc < 0:
            check(rc, "gpmpc_pack_autotune")
        self._drop_caches()
        out = []
        for item in buf.value.decode().split(";"):
            name, fields, ms = item.split(":")
            d = {"name": name.lstrip("*"), "winner": name.startswith("*"), "ms": float(ms)}
            for kv in fields.split(","):
                k, v = kv.split("=")
                d[k] = int(v)
            out.append(d)
        return out

    def autotune_clear(self):
        check(lib().gpmpc_pack_autotune_clear(self._h), "gpmpc_pack_autotune_clear")
        self._drop_caches()

    @property
    def shared_lambda(self):
        """True when every GP of the pack has bit-identical length-scales (the shared-lambda pair kernel applies)."""
        return lib().gpmpc_pack_shared_lambda(self._h) == 1

    @property
    def handle(self):
        return self._h

    def workspace(self, nbytes):
        """Scratch for one call, one buffer per stream: calls on different streams may overlap on the device (the C ABI is
        re-entrant across streams as long as the workspaces differ)."""
        key = torch.cuda.current_stream(self.device.index).cuda_stream
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            if ws is None and len(self._ws) >= 8:            # bounded: drop the workspace of the longest-unused stream
                torch.cuda.synchronize(self.device)
                self._ws.pop(next(iter(self._ws)))
            ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        else:
            self._ws.pop(key)
        self._ws[key] = ws                                   # most recently used last
        return ws

    def beta(self):
        """(ds, N) copy of the cached beta vectors (for tests)."""
        out = torch.empty((self.ds, self.Np), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().gpmpc_pack_export(self._h, ptr(out), None, stream_ptr()), "gpmpc_pack_export")
        return out[:, :self.N]

    def weights(self):
        """(ds, Np, Np) copy of the folded weight matrices, element (i<=j) at [a, j, i] (for tests)."""
        out = torch.empty((self.ds, self.Np, self.Np), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().gpmpc_pack_export(self._h, None, ptr(out), stream_ptr()), "gpmpc_pack_export")
        return out


def rollout(pack, x0, U, cost, want_grad=True, want_traj=True, graph=False, precision="fp64", constraints=None):
    """B shooting rollouts + cost (+ gradient) in one call (C ABI ``gpmpc_rollout``).

    constraints: a :class:`StateConstraints` -- the same device pass also returns g (B, H, m_c) and, with ``want_grad``, g_jac
    (B, H m_c, H da) (C ABI ``gpmpc_rollout_constrained``; fp64, no graph replay).  None: the function is exactly what it was.

    x0: (B, ds) or (ds,); U: (B, H, da) or (H, da).  Returns a dict of CUDA tensors:
    cost (B,), grad (B, H, da), means (B, H+1, ds), vars (B, H+1, ds).

    graph=True replays the 2H+1 kernel launches as one hipGraph (for launch-latency-bound small batches, e.g. the
    B = 1 callbacks of a solver loop): inputs are copied into buffers owned by the pack and the returned tensors are
    views of buffers that the NEXT graph call with the same shape overwrites.

    precision: "fp64" (default), or -- objective only, for the tolerance sweep of BASELINE config 3 -- "fp32acc" (N^2
    products and sum in fp32) / "fp32" (exponent and exp in fp32 too).  Single precision fails the variance tolerance
    by orders of magnitude (profiles/r01/fp32_sweep.txt); it is a measurement aid, not a fast path."""
    if constraints is not None:
        if graph or precision != "fp64":
            raise ValueError("a rollout with state constraints runs in fp64 as plain launches: graph=True and the reduced-precision modes "
                             "are not supported")
        return _rollout_constrained(pack, x0, U, cost, constraints, want_grad, want_traj)
    dev = pack.device
    U_host = None
    if graph and not isinstance(U, torch.Tensor):          # solver callbacks hand numpy: stage through pinned memory
        x0, U_host, B, H, da = _problem(pack, x0, np.ascontiguousarray(np.asarray(U, dtype=np.float64)), cost)
    else:
        x0, U, B, H, da = _problem(pack, x0, _dev(U, dev), cost)
    prec = {"fp64": 0, "fp32acc": _lib.FP32_ACCUM, "fp32": _lib.FP32_ALL}[precision]
    if prec and want_grad:
        raise ValueError("the reduced-precision sweep modes are objective only: pass want_grad=False")
    flags = (_lib.WANT_GRAD if want_grad else 0) | (_lib.USE_GRAPH if graph else 0) | prec
    nbytes = lib().gpmpc_rollout_workspace_bytes(pack.handle, B, H, flags)
    e = functools.partial(_empty, dev)
    if graph:
        key = (B, H, bool(want_grad), bool(want_traj))
        buf = pack._graph_bufs.get(key)
        if buf is None:
            # cost and grad are views of ONE block so that a caller can fetch both with a single device-to-host copy
            cg = e(B * (1 + (H * da if want_grad else 0)))
            buf = {"x0": e(B, pack.ds), "U": e(B, H, da), "cost_grad": cg, "cost": cg[:B],
                   "U_pinned": torch.empty((B, H, da), dtype=torch.float64).pin_memory(),
                   "ws": torch.empty(int(nbytes), dtype=torch.uint8, device=dev)}
            if want_grad:
                buf["grad"] = cg[B:].view(B, H, da)
            if want_traj:
                buf["means"], buf["vars"] = e(B, H + 1, pack.ds), e(B, H + 1, pack.ds)
            if len(pack._graph_bufs) >= 4:                   # the library keeps 4 captured shapes per pack
                pack._graph_bufs.pop(next(iter(pack._graph_bufs)))
            pack._graph_bufs[key] = buf
        if buf["ws"].numel() < nbytes:                          # the pack was refilled under a plan that needs more scratch
            buf["ws"] = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)     # (new pointer: the library captures anew)
        buf["x0"].copy_(x0)
        if U_host is not None:
            # the previous copy out of the pinned buffer has completed: every graph call is followed by a synchronising
            # read of its results before the next one can be issued from the same host thread
            torch.cuda.current_stream(dev).synchronize()
            buf["U_pinned"].numpy()[...] = U_host
            buf["U"].copy_(buf["U_pinned"], non_blocking=True)
        else:
            buf["U"].copy_(U)
        x0, U, ws = buf["x0"], buf["U"], buf["ws"]
        out = {k: buf[k] for k in ("cost", "grad", "means", "vars", "cost_grad") if k in buf}
    else:
        out = {"cost": e(B)}
        if want_grad:
            out["grad"] = e(B, H, da)
        if want_traj:
            out["means"], out["vars"] = e(B, H + 1, pack.ds), e(B, H + 1, pack.ds)
        ws = pack.workspace(nbytes)
    with torch.cuda.device(dev):
        check(lib().gpmpc_rollout(pack.handle, B, H, ptr(x0), ptr(U), ctypes.byref(cost.c), flags,
                                  ptr(out.get("means")), ptr(out.get("vars")), ptr(out["cost"]), ptr(out.get("grad")),
                                  ctypes.c_void_p(ws.data_ptr()), ws.numel(), stream_ptr()), "gpmpc_rollout")
    return out


def _rollout_constrained(pack, x0, U, cost, sc, want_grad, want_traj):
    dev = pack.device
    x0, U, B, H, da = _problem(pack, x0, _dev(U, dev), cost)
    if sc.ds != pack.ds:
        raise ValueError("the constraint rows have %d state coefficients, the pack has %d states" % (sc.ds, pack.ds))
    flags = _lib.WANT_GRAD if want_grad else 0
    e = functools.partial(_empty, dev)
    out = {"cost": e(B), "g": e(B, H, sc.m)}
    if want_grad:
        out["grad"], out["g_jac"] = e(B, H, da), e(B, H * sc.m, H * da)
    if want_traj:
        out["means"], out["vars"] = e(B, H + 1, pack.ds), e(B, H + 1, pack.ds)
    ws = pack.workspace(lib().gpmpc_rollout_constrained_workspace_bytes(pack.handle, B, H, flags))
    with torch.cuda.device(dev):
        check(lib().gpmpc_rollout_constrained(pack.handle, B, H, ptr(x0), ptr(U), ctypes.byref(cost.c), ctypes.byref(sc.c), flags,
                                              ptr(out.get("means")), ptr(out.get("vars")), ptr(out["cost"]), ptr(out.get("grad")),
                                              ptr(out["g"]), ptr(out.get("g_jac")), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                              stream_ptr()), "gpmpc_rollout_constrained")
    return out


def rollout_constraints(means, vars, jac, sc, ds, da):
    """Constraint values and Jacobian of given trajectories (C ABI ``gpmpc_rollout_constraints``; a pure function of what
    ``gpmpc_rollout_jac`` returns, any pack or plan).  means, vars: (B, H+1, ds); jac: (B, H, 2ds, 2ds+da) or None (values only).
    Returns {"g": (B, H, m_c)[, "g_jac": (B, H m_c, H da)]}."""
    dev = means.device if isinstance(means, torch.Tensor) and means.is_cuda else require_gpu()
    means, vars = _dev(means, dev), _dev(vars, dev)
    if means.dim() == 2:
        means, vars = means.unsqueeze(0), vars.unsqueeze(0)
    B, H1, ds_ = means.shape
    H = H1 - 1
    if ds_ != ds or sc.ds != ds or tuple(vars.shape) != (B, H1, ds):
        raise ValueError("shape mismatch between means, vars and the constraint rows")
    out = {"g": torch.empty((B, H, sc.m), dtype=torch.float64, device=dev)}
    if jac is not None:
        jac = _dev(jac, dev).reshape(B, H, 2 * ds, 2 * ds + da)
        out["g_jac"] = torch.empty((B, H * sc.m, H * da), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().gpmpc_rollout_constraints(B, H, ds, da, ctypes.byref(sc.c), ptr(means), ptr(vars), ptr(jac), ptr(out["g"]),
                                              ptr(out.get("g_jac")), stream_ptr()), "gpmpc_rollout_constraints")
    return out


def _fullcov_pack(pack):
    """What every full-covariance entry asks of a pack: no nominal model, cross-covariance weights."""
    if pack._nominal is not None:
        raise NotImplementedError("the full-covariance rollout does not support a pack with a linear nominal model "
                                  "(its cross-covariances with the linear part are not implemented)")
    if not pack.fullcov:
        pack.enable_fullcov()


def rollout_fullcov(pack, x0, U, cost, want_grad=True, constraints=None):
    """Like :func:`rollout` but propagating the FULL state covariance (C ABI ``gpmpc_rollout_fullcov``;
    BASELINE config 5).  Returns cost (B,), grad (B,H,da), means (B,H+1,ds), covs (B,H+1,ds,ds).

    constraints: a :class:`StateConstraints` -- the same device pass also returns g (B, H, m_c) under the full rule
    g[t, r] = A[r] . mu_t + kappa[r] sqrt(A[r]^T Sigma_t A[r]) - b[r] and, with ``want_grad``, g_jac (B, H m_c, H da) (C ABI
    ``gpmpc_rollout_fullcov_constrained``); cost, grad, means and covs keep their bits.  None: the function is exactly what it was."""
    dev = pack.device
    _fullcov_pack(pack)
    x0, U, B, H, da = _problem(pack, x0, _dev(U, dev), cost)
    flags = _lib.WANT_GRAD if want_grad else 0
    e = functools.partial(_empty, dev)
    out = {"cost": e(B), "means": e(B, H + 1, pack.ds), "covs": e(B, H + 1, pack.ds, pack.ds)}
    if want_grad:
        out["grad"] = e(B, H, da)
    if constraints is not None:
        sc = constraints
        if sc.ds != pack.ds:
            raise ValueError("the constraint rows have %d state coefficients, the pack has %d states" % (sc.ds, pack.ds))
        out["g"] = e(B, H, sc.m)
        if want_grad:
            out["g_jac"] = e(B, H * sc.m, H * da)
        ws = pack.workspace(lib().gpmpc_rollout_fullcov_constrained_workspace_bytes(pack.handle, B, H, flags))
        with torch.cuda.device(dev):
            check(lib().gpmpc_rollout_fullcov_constrained(pack.handle, B, H, ptr(x0), ptr(U), ctypes.byref(cost.c), ctypes.byref(sc.c), flags,
                                                          ptr(out["means"]), ptr(out["covs"]), ptr(out["cost"]), ptr(out.get("grad")),
                                                          ptr(out["g"]), ptr(out.get("g_jac")), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                                          stream_ptr()), "gpmpc_rollout_fullcov_constrained")
        return out
    nbytes = lib().gpmpc_rollout_fullcov_workspace_bytes(pack.handle, B, H, flags)
    ws = pack.workspace(nbytes)
    with torch.cuda.device(dev):
        check(lib().gpmpc_rollout_fullcov(pack.handle, B, H, ptr(x0), ptr(U), ctypes.byref(cost.c), flags,
                                          ptr(out["means"]), ptr(out["covs"]), ptr(out["cost"]), ptr(out.get("grad")),
                                          ctypes.c_void_p(ws.data_ptr()), ws.numel(), stream_ptr()),
              "gpmpc_rollout_fullcov")
    return out


def rollout_fullcov_jac(pack, x0, U):
    """Means, covariances and the PACKED step Jacobians of B full-covariance rollouts, no cost (C ABI ``gpmpc_rollout_fullcov_jac``, the
    counterpart of ``gpmpc_rollout_jac``).  x0: (B, ds) or (ds,); U: (B, H, da) or (H, da).  Returns means (B, H+1, ds), covs
    (B, H+1, ds, ds), jac (B, H, p, p + da) with p = ds + ds (ds + 1) / 2 in the convention of ``linearised.linearised_step_full``: what
    ``linearised.linearised_fc_vjp`` and ``linearised.linearised_fc_constraints`` take.  Not differentiable by autograd."""
    dev = pack.device
    _fullcov_pack(pack)
    U = _dev(U, dev)
    if U.ndim == 2:
        U = U[None]
    B, H, da = U.shape
    x0 = _dev(x0, dev).reshape(-1, pack.ds)
    if x0.shape[0] == 1 and B > 1:
        x0 = x0.expand(B, pack.ds).contiguous()
    if da != pack.da or x0.shape[0] != B:
        raise ValueError("shape mismatch between pack, x0 and U")
    ds = pack.ds
    p = ds + ds * (ds + 1) // 2
    e = functools.partial(_empty, dev)
    out = {"means": e(B, H + 1, ds), "covs": e(B, H + 1, ds, ds), "jac": e(B, H, p, p + da)}
    ws = pack.workspace(lib().gpmpc_rollout_fullcov_jac_workspace_bytes(pack.handle, B, H))
    with torch.cuda.device(dev):
        check(lib().gpmpc_rollout_fullcov_jac(pack.handle, B, H, ptr(x0), ptr(U), ptr(out["means"]), ptr(out["covs"]), ptr(out["jac"]),
                                              ctypes.c_void_p(ws.data_ptr()), ws.numel(), stream_ptr()), "gpmpc_rollout_fullcov_jac")
    return out


def moment_match(pack, u, S, want_cov=False, want_grad=False, bug_compatible=False, want_l=False):
    """Exact moment matching of all ds GPs for nq Gaussian inputs N(u, S) with full S
    (C ABI ``gpmpc_moment_match``).  u: (nq, D) or (D,); S: (nq, D, D) or (D, D)."""
    dev = pack.device
    if pack._nominal is not None:
        raise NotImplementedError("moment_match does not support a pack with a linear nominal model: it would return the moments of "
                                  "the residual GPs alone")
    u = _dev(u, dev).reshape(-1, pack.D)
    nq = u.shape[0]
    S = _dev(S, dev).reshape(nq, pack.D, pack.D)
    flags = (_lib.WANT_GRAD if want_grad else 0) | (_lib.COV_BUG_COMPAT if bug_compatible else 0)
    ds, D = pack.ds, pack.D
    e = functools.partial(_empty, dev)
    out = {"mean": e(nq, ds), "var": e(nq, ds)}
    if want_cov:
        out["cov"] = e(nq, ds, ds)
    if want_l:
        out["l"] = e(nq, ds, pack.N)
    if want_grad:
        out.update(dmean_du=e(nq, ds, D), dmean_dS=e(nq, ds, D, D), dvar_du=e(nq, ds, D), dvar_dS=e(nq, ds, D, D))
        if want_cov and ds > 1:
            # pair kernel's cross units when the pack has them (enable_fullcov) and the consistent form is asked for, else the direct
            # kernel (either form); the diagonal (a, a) entries are written too (= dvar_du / dvar_dS, by the variance units)
            out.update(dcov_du=torch.zeros((nq, ds, ds, D), dtype=torch.float64, device=dev),
                       dcov_dS=torch.zeros((nq, ds, ds, D, D), dtype=torch.float64, device=dev))
    nbytes = lib().gpmpc_moment_match_workspace_bytes(pack.handle, nq)
    ws = pack.workspace(nbytes)
    with torch.cuda.device(dev):
        check(lib().gpmpc_moment_match(pack.handle, nq, ptr(u), ptr(S), flags, ptr(out["mean"]), ptr(out["var"]),
                                       ptr(out.get("cov")), ptr(out.get("l")), ptr(out.get("dmean_du")), ptr(out.get("dmean_dS")),
                                       ptr(out.get("dvar_du")), ptr(out.get("dvar_dS")),
                                       ptr(out.get("dcov_du")), ptr(out.get("dcov_dS")),
                                       ctypes.c_void_p(ws.data_ptr()), ws.numel(), stream_ptr()), "gpmpc_moment_match")
    return out


def cost_full(cost, means, covs, U):
    """Risk-sensitive cost for given means (B,H+1,ds), FULL covariances (B,H+1,ds,ds), inputs (B,H,da)
    (C ABI ``gpmpc_cost``; reference src/mpc.py:156-200)."""
    dev = means.device if isinstance(means, torch.Tensor) and means.is_cuda else require_gpu()
    means, covs, U = _dev(means, dev), _dev(covs, dev), _dev(U, dev)
    if means.dim() == 2:
        means, covs, U = means.unsqueeze(0), covs.unsqueeze(0), U.unsqueeze(0)
    B, H1, ds = means.shape
    out = torch.empty(B, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().gpmpc_cost(B, H1 - 1, ds, U.shape[2], ctypes.byref(cost.c), ptr(means), ptr(covs), ptr(U), ptr(out),
                               stream_ptr()), "gpmpc_cost")
    return out
