"""Particles: the pointwise posterior of all GPs of a model at many points, and Monte-Carlo rollouts through it (C ABI "Particles" of
include/gpmpc.h).  No reference counterpart on the device: the reference checks its rollout against particles
through ``predict_latent_vars`` on the host (src/test/test_dynamics.py:198-268).

    model = GPModel.from_dynamics(dyn)              # dense (X_train, beta, Ky_inv in place) or sparse (Z, alpha, Q)
    mean, var = gp_posterior(model, Z)              # (nq, ds) each: all GPs at once
    r = particle_rollout(dyn, x0, U, particles=4096, constraints=sc)
    r["mean"], r["cov"], r["violation"], r["joint_violation"], r["clamped"], r["particles"]

Every call runs on the current stream of the model's device and returns device tensors; nothing synchronises."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import GPModelC, check, lib, ptr, stream_ptr, require_gpu
from .rollout import InputConstraints, StateConstraints, noise_arrays

_WS = {}                       # (device index, stream) -> workspace (grown, never shrunk)


def _workspace(device, nbytes):
    key = (device.index, torch.cuda.current_stream(device.index).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WS[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    return ws


def _dev(a, device):
    if isinstance(a, torch.Tensor):
        return a.detach().to(device=device, dtype=torch.float64).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64)), device=device)


class GPModel:
    """A GP bundle by raw arrays, as ``gpmpc_pack_build_beta`` / ``_strided`` take it: X (n, D), beta (n, ds), Kinv (n, n) -- one matrix
    for every GP, any row stride -- or (ds, n, n), lambdas (ds, D), sigma_f (ds,); optionally the linear nominal model (W (ds, D), b (ds,))
    and the noise model (init_cov, action_var, process_var; None: the defaults of ``GPPack.set_noise``).  Holds references to the tensors
    it points into; tensors given on the device are read in place."""

    def __init__(self, X, beta, Kinv, lambdas, sigma_f, state_dim, action_dim, nominal=None, init_cov=None, action_var=None, process_var=None,
                 device=None):
        ds, da = int(state_dim), int(action_dim)
        D = ds + da
        if not (1 <= ds <= _lib.MAX_DS and da >= 0 and D <= _lib.MAX_D):
            raise ValueError("state_dim in 1..%d and state_dim + action_dim <= %d are supported" % (_lib.MAX_DS, _lib.MAX_D))
        lam = np.asarray(lambdas, dtype=np.float64).reshape(ds, D)
        sf = np.broadcast_to(np.asarray(sigma_f, dtype=np.float64).reshape(-1), (ds,))
        self.device = device if device is not None else (X.device if isinstance(X, torch.Tensor) and X.is_cuda else require_gpu())
        self.X = _dev(X, self.device).reshape(-1, D)
        n = self.X.shape[0]
        self.beta = _dev(beta, self.device).reshape(n, ds)
        K = Kinv if isinstance(Kinv, torch.Tensor) and Kinv.is_cuda and Kinv.dtype == torch.float64 else _dev(Kinv, self.device)
        K = K.detach()
        if K.dim() == 2:
            if K.shape != (n, n):
                raise ValueError("Kinv: (%d, %d) or (%d, %d, %d), got %s" % (n, n, ds, n, n, tuple(K.shape)))
            if K.stride(1) != 1 and n > 1:
                K = K.contiguous()
            ld, gp_stride = (K.stride(0) if n > 1 else max(K.stride(0), 1)), 0
        else:
            if tuple(K.shape) != (ds, n, n):
                raise ValueError("Kinv: (%d, %d) or (%d, %d, %d), got %s" % (n, n, ds, n, n, tuple(K.shape)))
            K = K.contiguous()
            ld, gp_stride = n, n * n
        self.Kinv = K
        self.n, self.ds, self.da, self.D = n, ds, da, D
        self.lambdas, self.sigma_f = lam.copy(), sf.copy()
        c = GPModelC()
        c.n, c.state_dim, c.action_dim = n, ds, da
        c.X, c.beta, c.Kinv = self.X.data_ptr(), self.beta.data_ptr(), K.data_ptr()
        c.ld, c.gp_stride = int(ld), int(gp_stride)
        c.lambdas[:ds * D] = lam.reshape(-1).tolist()
        c.sigma_f[:ds] = sf.tolist()
        self.nominal = None
        if nominal is not None:
            W = np.asarray(nominal[0], dtype=np.float64).reshape(ds, D)
            b = np.broadcast_to(np.asarray(nominal[1], dtype=np.float64).reshape(-1), (ds,))
            c.has_nominal = 1
            c.nom_w[:ds * D] = W.reshape(-1).tolist()
            c.nom_b[:ds] = b.tolist()
            self.nominal = (W.copy(), b.copy())
        P, av, pv = noise_arrays(ds, da, init_cov, action_var, process_var)
        self.noise = None
        if P is not None or av is not None or pv is not None:
            P = np.eye(ds) * 1e-3 if P is None else P
            av = np.full(da, float(np.float32(1e-3))) if av is None else av
            pv = np.zeros(ds) if pv is None else pv
            c.has_noise = 1
            c.init_cov[:ds * ds] = P.reshape(-1).tolist()
            c.action_var[:da] = np.asarray(av).reshape(-1).tolist()
            c.process_var[:ds] = pv.tolist()
            self.noise = (P, av, pv)
        self.c = c

    @classmethod
    def from_dynamics(cls, dyn):
        """The model a ``Dynamics`` (dense: X_train, beta(), Ky_inv in place -- ONE inverse when the GPs share it, as ``Dynamics.pack()``
        detects) or a ``SparseDynamics`` (Z, alpha, Q of ``posterior()``) holds now, with its linear nominal model and its noise model."""
        ds, da = dyn.state_dim, dyn.action_dim
        lam = np.stack([g.get_lambdas() for g in dyn.gpr_err])
        sf = np.array([g.get_sigma_f() for g in dyn.gpr_err])
        if hasattr(dyn, "posterior"):
            beta, Kinv = dyn.posterior()
            X = torch.as_tensor(dyn.inducing, device=dyn.device)
            nominal = dyn._nominal_arrays()
        else:
            g0 = dyn.gpr_err[0]
            if g0.num_train == 0:
                raise RuntimeError("no training data")
            nominal = dyn._linear_nominal()
            X = g0.X_train
            if dyn.nominal_models is None or nominal is not None:
                beta = torch.stack([g.beta() for g in dyn.gpr_err], dim=1)      # (of the residual of a linear model, where there is one)
            else:                                        # other callables: the rollout runs the zero-mean GPs on the raw targets, and so do we
                beta = torch.stack([g.Ky_inv @ g.y_train.reshape(-1) for g in dyn.gpr_err], dim=1)
            if all(g.Ky_inv is g0.Ky_inv for g in dyn.gpr_err):
                Kinv = g0.Ky_inv
            else:
                Kinv = torch.stack([g.Ky_inv.detach() for g in dyn.gpr_err])
        nm = getattr(dyn, "_noise", None)
        P = av = pv = None
        if nm is not None:
            P, av, pv = nm
            if isinstance(pv, str):
                pv = np.array([float(g.get_sigma_n()) ** 2 for g in dyn.gpr_err])
        return cls(X, beta, Kinv, lam, sf, ds, da, nominal=nominal, init_cov=P, action_var=av, process_var=pv, device=dyn.device)


def _model(m):
    return m if isinstance(m, GPModel) else GPModel.from_dynamics(m)


def _empty(device, *shape, dtype=torch.float64):
    return torch.empty(shape, dtype=dtype, device=device)


def _vp(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def gp_posterior(model, Z, chunk=0):
    """(mean (nq, ds), var (nq, ds)) of all GPs at the points Z (nq, D): the latent variance sf^2 - k*^T Kinv k* + process_var, unclamped."""
    model = _model(model)
    Z = _dev(Z, model.device).reshape(-1, model.D)
    nq = Z.shape[0]
    mean, var = _empty(model.device, nq, model.ds), _empty(model.device, nq, model.ds)
    with torch.cuda.device(model.device):
        nb = lib().gpmpc_gp_posterior_workspace_bytes(ctypes.byref(model.c), nq, chunk)
        ws = _workspace(model.device, nb)
        check(lib().gpmpc_gp_posterior(ctypes.byref(model.c), nq, ptr(Z), ptr(mean), ptr(var), chunk, _vp(ws), nb, stream_ptr(model.device)),
              "gpmpc_gp_posterior")
    return mean, var


def particle_noise(P, n_normals, t, seed=0, call_index=0, device=None):
    """The normals (P, n_normals) the rollout uses at step t (ds of them at t = 0, da + ds at t >= 1)."""
    device = device if device is not None else require_gpu()
    out = _empty(device, int(P), int(n_normals))
    with torch.cuda.device(device):
        check(lib().gpmpc_particle_noise(int(P), int(n_normals), int(t), int(seed) & (2 ** 64 - 1), int(call_index), ptr(out), stream_ptr(device)),
              "gpmpc_particle_noise")
    return out


def particle_step(model, x_prev, U_t, eps, chunk=0, return_moments=False):
    """One step: x_prev (B, P, ds), U_t (B, da), eps (P, da + ds) -> x_next (B, P, ds) [, mean, var of the same shape]."""
    model = _model(model)
    x_prev = _dev(x_prev, model.device)
    B, P = x_prev.shape[0], x_prev.shape[1]
    U_t = _dev(U_t, model.device).reshape(B, model.da)
    eps = _dev(eps, model.device).reshape(P, model.da + model.ds)
    nxt = _empty(model.device, B, P, model.ds)
    mean = _empty(model.device, B, P, model.ds) if return_moments else None
    var = _empty(model.device, B, P, model.ds) if return_moments else None
    with torch.cuda.device(model.device):
        nb = lib().gpmpc_particle_step_workspace_bytes(ctypes.byref(model.c), B, P, chunk)
        ws = _workspace(model.device, nb)
        check(lib().gpmpc_particle_step(ctypes.byref(model.c), B, P, ptr(x_prev), _vp(U_t) if model.da else None, model.da, ptr(eps), ptr(nxt),
                                        _vp(mean), _vp(var), chunk, _vp(ws), nb, stream_ptr(model.device)), "gpmpc_particle_step")
    return (nxt, mean, var) if return_moments else nxt


def particle_stats(particles, var=None, constraints=None):
    """particles (T, B, P, ds) [, var of the same shape] -> dict(mean (B, T, ds), cov (B, T, ds, ds) [, clamped (B, T) int32]
    [, violation (B, T, rows), joint_violation (B,)])."""
    assert particles.is_cuda and particles.dtype == torch.float64 and particles.is_contiguous()
    T, B, P, ds = particles.shape
    dev = particles.device
    out = {"mean": _empty(dev, B, T, ds), "cov": _empty(dev, B, T, ds, ds)}
    clamped = _empty(dev, B, T, dtype=torch.int32) if var is not None else None
    sc = constraints
    viol = _empty(dev, B, T, sc.m) if sc is not None else None
    joint = _empty(dev, B) if sc is not None else None
    with torch.cuda.device(dev):
        check(lib().gpmpc_particle_stats(B, P, T, ds, ptr(particles), _vp(var), ctypes.byref(sc.c) if sc is not None else None,
                                         ptr(out["mean"]), ptr(out["cov"]), _vp(clamped), _vp(viol), _vp(joint), stream_ptr(dev)),
              "gpmpc_particle_stats")
    if var is not None:
        out["clamped"] = clamped
    if sc is not None:
        out["violation"], out["joint_violation"] = viol, joint
    return out


def particle_inputs(x_prev, U_t, K_t=None, mu_t=None):
    """The inputs of particles under a state feedback (C ABI ``gpmpc_particle_inputs``): x_prev (B, P, ds), U_t (B, da), K_t (da, ds) or
    None (a copy of U_t per particle), mu_t (B, ds) -> u (B, P, da) = U_t + K_t (x - mu_t)."""
    dev = x_prev.device
    B, P, ds = x_prev.shape
    x_prev, U_t = x_prev.contiguous(), _dev(U_t, dev).reshape(B, -1).contiguous()
    da = U_t.shape[1]
    K_t = None if K_t is None else _dev(K_t, dev).reshape(da, ds).contiguous()
    mu_t = None if mu_t is None else _dev(mu_t, dev).reshape(B, ds).contiguous()
    out = _empty(dev, B, P, da)
    with torch.cuda.device(dev):
        check(lib().gpmpc_particle_inputs(B, P, ds, da, ptr(x_prev), ptr(U_t), da, _vp(K_t), _vp(mu_t), ds, ptr(out), stream_ptr(dev)),
              "gpmpc_particle_inputs")
    return out


def particle_step_inputs(model_or_dynamics, x_prev, U_p, eps, chunk=0):
    """``particle_step`` with an input per particle (C ABI ``gpmpc_particle_step_inputs``): x_prev (B, P, ds), U_p (B, P, da) (what
    ``particle_inputs`` returns), eps (P, da + ds) -> (next (B, P, ds), mean, var (B, P, ds))."""
    model = _model(model_or_dynamics)
    ds, da, dev = model.ds, model.da, model.device
    B, P = x_prev.shape[0], x_prev.shape[1]
    x_prev, U_p, eps = _dev(x_prev, dev).contiguous(), _dev(U_p, dev).reshape(B, P, da).contiguous(), _dev(eps, dev).reshape(P, da + ds).contiguous()
    nxt, mean, var = _empty(dev, B, P, ds), _empty(dev, B, P, ds), _empty(dev, B, P, ds)
    with torch.cuda.device(dev):
        nb = lib().gpmpc_particle_step_inputs_workspace_bytes(ctypes.byref(model.c), B, P, chunk)
        ws = _workspace(dev, nb)
        check(lib().gpmpc_particle_step_inputs(ctypes.byref(model.c), B, P, ptr(x_prev), ptr(U_p), ptr(eps), ptr(nxt), ptr(mean), ptr(var), chunk,
                                               _vp(ws), nb, stream_ptr(dev)), "gpmpc_particle_step_inputs")
    return nxt, mean, var


def particle_input_stats(inputs, input_constraints=None):
    """Statistics of particle inputs (C ABI ``gpmpc_particle_input_stats``): inputs (H, B, P, da) -> dict(input_mean (B, H, da), input_cov
    (B, H, da, da) and, with an ``InputConstraints``, input_violation (B, H, rows), joint_input_violation (B,))."""
    dev = inputs.device
    H, B, P, da = inputs.shape
    ic = input_constraints
    out = {"input_mean": _empty(dev, B, H, da), "input_cov": _empty(dev, B, H, da, da)}
    if ic is not None:
        out["input_violation"], out["joint_input_violation"] = _empty(dev, B, H, ic.m), _empty(dev, B)
    with torch.cuda.device(dev):
        check(lib().gpmpc_particle_input_stats(B, P, H, da, ptr(inputs.contiguous()), ctypes.byref(ic.c) if ic is not None else None,
                                               ptr(out["input_mean"]), ptr(out["input_cov"]), _vp(out.get("input_violation")),
                                               _vp(out.get("joint_input_violation")), stream_ptr(dev)), "gpmpc_particle_input_stats")
    return out


def particle_rollout(model_or_dynamics, x0, U, particles=1024, seed=0, call_index=0, constraints=None, return_particles=True, chunk=0,
                     feedback=None, mean_ref=None, input_constraints=None):
    """Monte-Carlo rollout of B plans with ``particles`` particles each through the GP posterior (every plan sees the same noise).
    x0 (ds,) or (B, ds); U (H, da) or (B, H, da); constraints: a ``StateConstraints`` (its rows a . x <= b are counted; kappa is not used).
    Returns device tensors: ``particles`` (B, P, H+1, ds) (a view), ``mean`` (B, H+1, ds), ``cov`` (B, H+1, ds, ds) (divisor P - 1),
    ``clamped`` (B, H) int32 -- particles whose latent variance came out negative at a step --, and with constraints ``violation``
    (B, H+1, rows), the fraction of particles with a . x > b, and ``joint_violation`` (B,), the fraction violating any row at any step >= 1.
    feedback=K ((da, ds) or (H, da, ds)) with mean_ref (B, H+1, ds) (or (H+1, ds)), and / or input_constraints (an ``InputConstraints``): the
    particles run under u = U_t + K_t (x - mean_ref_t) (C ABI ``gpmpc_particle_rollout_feedback``; the same noise, no new normals), and the
    result also holds ``inputs`` (B, P, H, da) (a view), ``input_mean`` (B, H, da), ``input_cov`` (B, H, da, da) and, with input rows,
    ``input_violation`` (B, H, rows) and ``joint_input_violation`` (B,) over the steps 0 ... H-1."""
    model = _model(model_or_dynamics)
    ds, da, dev = model.ds, model.da, model.device
    U = _dev(U, dev)
    if U.dim() == 2:
        U = U[None]
    B, H = U.shape[0], U.shape[1]
    U = U.reshape(B, H, da).contiguous()
    x0 = _dev(x0, dev).reshape(-1, ds)
    if x0.shape[0] == 1 and B > 1:
        x0 = x0.expand(B, ds).contiguous()
    if x0.shape[0] != B:
        raise ValueError("x0: (%d,) or (%d, %d), got %s" % (ds, B, ds, tuple(x0.shape)))
    if constraints is not None and not isinstance(constraints, StateConstraints):
        raise TypeError("constraints: a StateConstraints")
    if constraints is not None and constraints.ds != ds:
        raise ValueError("constraint rows have %d columns, the state %d" % (constraints.ds, ds))
    P, sc = int(particles), constraints
    part = _empty(dev, H + 1, B * P, ds)
    out = {"mean": _empty(dev, B, H + 1, ds), "cov": _empty(dev, B, H + 1, ds, ds), "clamped": _empty(dev, B, H, dtype=torch.int32)}
    viol = _empty(dev, B, H + 1, sc.m) if sc is not None else None
    joint = _empty(dev, B) if sc is not None else None
    ic = input_constraints
    if ic is not None and not isinstance(ic, InputConstraints):
        raise TypeError("input_constraints: an InputConstraints")
    if ic is not None and ic.da != da:
        raise ValueError("the input constraint rows have %d coefficients, the model has %d inputs" % (ic.da, da))
    if feedback is not None or ic is not None or mean_ref is not None:
        K = kstride = mu = None
        if feedback is not None:
            K = _dev(feedback, dev)
            if tuple(K.shape) not in ((da, ds), (H, da, ds)) or da == 0:
                raise ValueError("feedback gain: (%d, %d) or (%d, %d, %d), got %s" % (da, ds, H, da, ds, tuple(K.shape)))
            if mean_ref is None:
                raise ValueError("a feedback gain needs mean_ref, the mean trajectory it acts around")
        kstride = da * ds if K is not None and K.dim() == 3 else 0
        if mean_ref is not None:
            mu = _dev(mean_ref, dev).reshape(-1, H + 1, ds)
            if mu.shape[0] == 1 and B > 1:
                mu = mu.expand(B, H + 1, ds)
            if mu.shape[0] != B:
                raise ValueError("mean_ref: (%d, %d) or (%d, %d, %d), got %s" % (H + 1, ds, B, H + 1, ds, tuple(mu.shape)))
            mu = mu.contiguous()
        inp = _empty(dev, H, B * P, da)
        out["input_mean"], out["input_cov"] = _empty(dev, B, H, da), _empty(dev, B, H, da, da)
        if ic is not None:
            out["input_violation"], out["joint_input_violation"] = _empty(dev, B, H, ic.m), _empty(dev, B)
        with torch.cuda.device(dev):
            nb = lib().gpmpc_particle_rollout_feedback_workspace_bytes(ctypes.byref(model.c), B, P, H, chunk, 1)
            ws = _workspace(dev, nb)
            check(lib().gpmpc_particle_rollout_feedback(
                ctypes.byref(model.c), B, P, H, ptr(x0), _vp(U) if da else None, int(seed) & (2 ** 64 - 1), int(call_index),
                ctypes.byref(sc.c) if sc is not None else None, ptr(part), ptr(out["mean"]), ptr(out["cov"]), _vp(out["clamped"]), _vp(viol),
                _vp(joint), _vp(K.contiguous() if K is not None else None), kstride, _vp(mu), ctypes.byref(ic.c) if ic is not None else None,
                ptr(inp), ptr(out["input_mean"]), ptr(out["input_cov"]), _vp(out.get("input_violation")), _vp(out.get("joint_input_violation")),
                chunk, _vp(ws), nb, stream_ptr(dev)), "gpmpc_particle_rollout_feedback")
        out["inputs"] = inp.reshape(H, B, P, da).permute(1, 2, 0, 3)
        if sc is not None:
            out["violation"], out["joint_violation"] = viol, joint
        if return_particles:
            out["particles"] = part.reshape(H + 1, B, P, ds).permute(1, 2, 0, 3)
        out["model"] = model
        return out
    with torch.cuda.device(dev):
        nb = lib().gpmpc_particle_rollout_workspace_bytes(ctypes.byref(model.c), B, P, H, chunk)
        ws = _workspace(dev, nb)
        check(lib().gpmpc_particle_rollout(ctypes.byref(model.c), B, P, H, ptr(x0), _vp(U) if da else None, int(seed) & (2 ** 64 - 1),
                                           int(call_index), ctypes.byref(sc.c) if sc is not None else None, ptr(part), ptr(out["mean"]),
                                           ptr(out["cov"]), _vp(out["clamped"]), _vp(viol), _vp(joint), chunk, _vp(ws), nb, stream_ptr(dev)),
              "gpmpc_particle_rollout")
    if sc is not None:
        out["violation"], out["joint_violation"] = viol, joint
    if return_particles:
        out["particles"] = part.reshape(H + 1, B, P, ds).permute(1, 2, 0, 3)
    out["model"] = model                                 # (keeps the tensors the call read alive until the caller drops the result)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# Particle cost (C ABI "Particle cost" of include/gpmpc.h): the entropic risk of the stage cost and empirical quantiles
# of the constraint margins ON the particles, the streaming evaluation, and MPPI over it.
#
#     r = particle_evaluate(dyn, x0, U, cost, constraints=sc, particles=256)       # r["cost"] (B,), r["stage"] (B, H+1), r["g"] (B, H, rows)
#     s = mppi_solve_particles(dyn, x0, U0, cost, constraints=sc, particles=256, samples=64)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _check_rows(constraints, ds):
    if constraints is not None and not isinstance(constraints, StateConstraints):
        raise TypeError("constraints: a StateConstraints")
    if constraints is not None and constraints.ds != ds:
        raise ValueError("constraint rows have %d columns, the state %d" % (constraints.ds, ds))


def particle_cost(particles, U, cost, constraints=None):
    """The particle cost of stored particles (C ABI ``gpmpc_particle_cost``): particles (H+1, B, P, ds) -- ``particle_rollout``'s
    ``particles`` permuted to (2, 0, 1, 3) -- or (H+1, B P, ds) with U (B, H, da); cost: a ``CostParams``.  Returns dict(cost (B,),
    stage (B, H+1) [, g (B, H, rows)]): J_b = sum_i s_i + the input terms of ``gpmpc_cost``, s_i the entropic risk (gamma != 0) or the mean
    (gamma == 0) of e^T Q e over the particles of step i, g the (P - m_r)-th smallest margin a_r . x - b_r with m_r = floor(eps_r P + 1e-9)."""
    assert particles.is_cuda and particles.dtype == torch.float64 and particles.is_contiguous()
    dev = particles.device
    U = _dev(U, dev)
    if U.dim() == 2:
        U = U[None]
    B, H, da = U.shape
    U = U.contiguous()
    T, ds = particles.shape[0], particles.shape[-1]
    if T != H + 1 or particles.numel() % (T * B * ds):
        raise ValueError("particles: (H+1, B, P, ds) for U (B, H, da), got %s and %s" % (tuple(particles.shape), tuple(U.shape)))
    P = particles.numel() // (T * B * ds)
    if cost.ds != ds or cost.da != da:
        raise ValueError("shape mismatch between particles, U and cost parameters")
    _check_rows(constraints, ds)
    sc = constraints
    out = {"cost": _empty(dev, B), "stage": _empty(dev, B, H + 1)}
    g = _empty(dev, B, H, sc.m) if sc is not None else None
    with torch.cuda.device(dev):
        check(lib().gpmpc_particle_cost(B, P, H, ds, da, ctypes.byref(cost.c), ctypes.byref(sc.c) if sc is not None else None, ptr(particles),
                                        _vp(U) if da else None, ptr(out["cost"]), ptr(out["stage"]), _vp(g), stream_ptr(dev)),
              "gpmpc_particle_cost")
    if sc is not None:
        out["g"] = g
    return out


def particle_evaluate(model_or_dynamics, x0, U, cost, constraints=None, particles=256, seed=0, call_index=0, chunk=0):
    """Rollout and particle cost in one pass that never stores the horizon (C ABI ``gpmpc_particle_evaluate``): bit for bit
    ``particle_cost`` on the particles ``particle_rollout`` stores for the same (seed, call_index).  x0 (ds,) or (B, ds); U (H, da) or
    (B, H, da).  Returns dict(cost (B,), stage (B, H+1), g (B, H, rows) or None)."""
    model = _model(model_or_dynamics)
    ds, da, dev = model.ds, model.da, model.device
    U = _dev(U, dev)
    if U.dim() == 2:
        U = U[None]
    B, H = U.shape[0], U.shape[1]
    U = U.reshape(B, H, da).contiguous()
    x0 = _dev(x0, dev).reshape(-1, ds)
    if x0.shape[0] == 1 and B > 1:
        x0 = x0.expand(B, ds).contiguous()
    if x0.shape[0] != B:
        raise ValueError("x0: (%d,) or (%d, %d), got %s" % (ds, B, ds, tuple(x0.shape)))
    if cost.ds != ds or cost.da != da:
        raise ValueError("shape mismatch between model and cost parameters")
    _check_rows(constraints, ds)
    P, sc = int(particles), constraints
    out = {"cost": _empty(dev, B), "stage": _empty(dev, B, H + 1), "g": _empty(dev, B, H, sc.m) if sc is not None else None}
    with torch.cuda.device(dev):
        nb = lib().gpmpc_particle_evaluate_workspace_bytes(ctypes.byref(model.c), B, P, H, chunk)
        ws = _workspace(dev, nb)
        check(lib().gpmpc_particle_evaluate(ctypes.byref(model.c), B, P, H, ptr(x0), _vp(U) if da else None, int(seed) & (2 ** 64 - 1),
                                            int(call_index), ctypes.byref(cost.c), ctypes.byref(sc.c) if sc is not None else None,
                                            ptr(out["cost"]), ptr(out["stage"]), _vp(out["g"]), chunk, _vp(ws), nb, stream_ptr(dev)),
              "gpmpc_particle_evaluate")
    out["model"] = model
    return out


def mppi_solve_particles(model_or_dynamics, x0, U0, cost, constraints=None, particles=256, samples=64, iterations=30, sigma=1.0, decay=0.9,
                         beta=0.1, seed=0, call_index=0, lb=None, ub=None):
    """``mppi.mppi_solve`` over the particle cost (C ABI ``gpmpc_mppi_solve_particles``): per iteration the sample kernel,
    ``gpmpc_particle_evaluate`` over the K samples with ``particles`` particles each, the update kernel; the whole search one enqueue,
    one device-to-host copy at the end.  The particle noise is that of (seed, call_index) and THE SAME in every iteration (common random
    numbers: the search minimises one fixed sample-average objective).  Returns what ``mppi_solve`` returns."""
    from ._solver import model_problem, mppi_result, mppi_result_block
    from .mppi import mppi_params
    model = _model(model_or_dynamics)
    dev = model.device
    x0, U0 = model_problem(model, x0, U0, cost)
    H, da = U0.shape
    _check_rows(constraints, model.ds)
    Pm = mppi_params(samples, da, sigma, lb, ub, iterations=iterations, decay=decay, beta=beta, seed=seed, call_index=call_index)
    cons = None if constraints is None else ctypes.byref(constraints.c)
    n = H * da
    res = mppi_result_block(n, Pm.iterations, dev)
    with torch.cuda.device(dev):
        nb = lib().gpmpc_mppi_solve_particles_workspace_bytes(ctypes.byref(model.c), H, int(particles), ctypes.byref(Pm), cons)
        ws = _workspace(dev, nb)
        check(lib().gpmpc_mppi_solve_particles(ctypes.byref(model.c), H, int(particles), ptr(x0), ptr(U0.contiguous()), ctypes.byref(cost.c), cons,
                                               ctypes.byref(Pm), ptr(res[:n]), ptr(res[n:n + 2]), ptr(res[n + 2:]), _vp(ws), ws.numel(),
                                               stream_ptr(dev)), "gpmpc_mppi_solve_particles")
    return mppi_result(res.cpu().numpy(), H, da)
