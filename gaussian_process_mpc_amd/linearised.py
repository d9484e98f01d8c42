"""Linearised (first-order, "mean-equivalent") uncertainty propagation on the device (C ABI "Linearised propagation" of include/gpmpc.h,
kernels in csrc/linprop.hip): mu' = m(z), v' = s2(z) + sum_d (dm/dz_d)^2 S_d at z = (mu, u).  Its O(N^2) part is one
quadratic form per plan, GP and step -- a matrix product on the MFMA pipe, not a per-pair exp as in exact moment matching.

    model = GPModel.from_dynamics(dyn)                       # dense or sparse, with its nominal and noise model
    mu1, var1, jac = linearised_step(model, mu, var, U_t)
    r = linearised_rollout(dyn, x0, U, cost)                 # what rollout(pack, x0, U, cost) returns, by the other rule
    s = mppi_solve_linearised(model, x0, U0, cost, samples=1024)

Two forms of the step (C ABI ``gpmpc_linearised_set_form``): "tile", the 64-column MFMA kernels and the default; "stream", matrix-vector
kernels for a few columns (csrc/linprop_stream.hip); "auto", stream up to ``LINPROP_AUTO_MAX_B`` columns.  ``with linearised_form("stream"):``
selects one for a block; every entry also takes ``form=``.

The full-covariance rule with a linear state feedback u = v + K (x - mu) (C ABI "Linearised propagation, full covariance", kernels in
csrc/linprop_fc.hip):

    mu1, cov1, jac = linearised_step_full(model, mu, cov, U_t, K_t)   # jac over the packed state (mu, Sigma_kl for k <= l)
    K = lqr_gain(model, x_eq, u_eq, Q, R)
    r = linearised_rollout(dyn, x0, U, cost, constraints=sc, full_covariance=True, feedback=K)    # covs in the place of vars

Plumbing only: the arithmetic is in the kernels (lqr_gain's Riccati recursion is host numpy).  Every call runs on the current stream of the model's device and returns device tensors."""
import contextlib
import ctypes

import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from ._solver import model_problem, mppi_result, mppi_result_block
from .mppi import mppi_params
from .particles import GPModel, _dev, _empty, _model, _vp, _workspace
from .rollout import InputConstraints, StateConstraints


FORMS = {"tile": _lib.LINPROP_FORM_TILE, "stream": _lib.LINPROP_FORM_STREAM, "auto": _lib.LINPROP_FORM_AUTO}


def _form_code(name):
    if name is not None and name not in FORMS:
        raise ValueError("form must be None, 'tile', 'stream' or 'auto', got %r" % (name,))
    return None if name is None else FORMS[name]


@contextlib.contextmanager
def linearised_form(name):
    """Selects the form of the linearised step for the block -- "tile", "stream" or "auto"; None leaves the process-wide choice alone -- and
    restores the previous one on the way out, also on an exception.  An unknown name raises ValueError before anything is set.  The library
    reads the form on the host when a call is ENQUEUED, not when its kernels run, so setting and restoring around asynchronous launches is
    sound: what was enqueued inside the block keeps the form it was enqueued with.  The choice is process-wide (not per thread)."""
    code = _form_code(name)
    if code is None:
        yield
        return
    old = lib().gpmpc_linearised_set_form(code)
    try:
        yield
    finally:
        lib().gpmpc_linearised_set_form(old)


def linearised_step(model, mu, var, U_t, want_jac=True, chunk=0, form=None):
    """One step of B plans: mu, var (B, ds), U_t (B, da) -> (mu', var') or, with ``want_jac``, (mu', var', jac (B, 2ds, 2ds+da)): rows
    (mu', var'), columns (mu, var, u), the layout of ``gpmpc_rollout_jac``.  form: see ``linearised_form``."""
    _form_code(form)
    model = _model(model)
    ds, da, dev = model.ds, model.da, model.device
    mu = _dev(mu, dev).reshape(-1, ds)
    B = mu.shape[0]
    var = _dev(var, dev).reshape(B, ds)
    U_t = _dev(U_t, dev).reshape(B, da) if da else None
    out_mu, out_var = _empty(dev, B, ds), _empty(dev, B, ds)
    nz, nc = 2 * ds, 2 * ds + da
    jac = _empty(dev, B, nz, nc) if want_jac else None
    with torch.cuda.device(dev), linearised_form(form):
        nb = lib().gpmpc_linearised_step_workspace_bytes(ctypes.byref(model.c), B, 1 if want_jac else 0, chunk)
        ws = _workspace(dev, nb)
        check(lib().gpmpc_linearised_step(ctypes.byref(model.c), B, ptr(mu), ptr(var), _vp(U_t) if da else None, da, ptr(out_mu), ptr(out_var),
                                          _vp(jac), nz * nc, chunk, _vp(ws), nb, stream_ptr(dev)), "gpmpc_linearised_step")
    return (out_mu, out_var, jac) if want_jac else (out_mu, out_var)


def packed_dim(ds):
    """p = ds + ds (ds + 1) / 2: the length of the packed state (mu, Sigma_kl for k <= l, row-major) of the full-covariance rule."""
    return ds + ds * (ds + 1) // 2


def _gain(K, H, ds, da, dev):
    """A feedback gain as (device tensor or None, k_step_stride): (da, ds) for every step, or (H, da, ds)."""
    if K is None:
        return None, 0
    K = _dev(K, dev)
    if da == 0:
        raise ValueError("a feedback gain needs action_dim >= 1")
    if tuple(K.shape) == (da, ds):
        return K.contiguous(), 0
    if H is not None and tuple(K.shape) == (H, da, ds):
        return K.contiguous(), da * ds
    raise ValueError("feedback gain: (%d, %d)%s, got %s" % (da, ds, "" if H is None else " or (%d, %d, %d)" % (H, da, ds), tuple(K.shape)))


def linearised_step_full(model, mu, cov, U_t, K_t=None, want_jac=True, chunk=0, form=None):
    """One step of the full-covariance linearised rule under the feedback u = U_t + K_t (x - mu) (C ABI ``gpmpc_linearised_fc_step``):
    mu (B, ds), cov (B, ds, ds) (the upper triangle is read), U_t (B, da), K_t (da, ds) or None -> (mu', cov') or, with ``want_jac``,
    (mu', cov', jac (B, p, p + da)) over the packed state (mu, Sigma_kl for k <= l), p = ``packed_dim(ds)``: rows s', columns (s, v).
    form: see ``linearised_form`` (the O(N^2) part is the diagonal step's own kernels)."""
    _form_code(form)
    model = _model(model)
    ds, da, dev = model.ds, model.da, model.device
    mu = _dev(mu, dev).reshape(-1, ds).contiguous()
    B = mu.shape[0]
    cov = _dev(cov, dev).reshape(B, ds, ds).contiguous()
    U_t = _dev(U_t, dev).reshape(B, da).contiguous() if da else None
    K_t, _ = _gain(K_t, None, ds, da, dev)
    out_mu, out_cov = _empty(dev, B, ds), _empty(dev, B, ds, ds)
    p = packed_dim(ds)
    jac = _empty(dev, B, p, p + da) if want_jac else None
    with torch.cuda.device(dev), linearised_form(form):
        nb = lib().gpmpc_linearised_fc_step_workspace_bytes(ctypes.byref(model.c), B, 1 if want_jac else 0, chunk)
        ws = _workspace(dev, nb)
        check(lib().gpmpc_linearised_fc_step(ctypes.byref(model.c), B, ptr(mu), ptr(cov), _vp(U_t) if da else None, da, _vp(K_t), ptr(out_mu),
                                             ptr(out_cov), _vp(jac), p * (p + da), chunk, _vp(ws), nb, stream_ptr(dev)),
              "gpmpc_linearised_fc_step")
    return (out_mu, out_cov, jac) if want_jac else (out_mu, out_cov)


def linearised_fc_vjp(jac, g_means, g_covs, ds, da, want_gx0=False):
    """The adjoint sweep over packed step Jacobians (C ABI ``gpmpc_linearised_fc_vjp``; a pure function of a propagated trajectory):
    jac (B, H, p, p + da), g_means (B, H+1, ds) or None, g_covs (B, H+1, ds, ds) or None -> gU (B, H, da) [, gx0 (B, ds)]."""
    B, H = jac.shape[0], jac.shape[1]
    dev = jac.device
    gU = _empty(dev, B, H, da)
    gx0 = _empty(dev, B, ds) if want_gx0 else None
    with torch.cuda.device(dev):
        check(lib().gpmpc_linearised_fc_vjp(B, H, ds, da, ptr(jac), _vp(g_means), _vp(g_covs), ptr(gU), _vp(gx0), stream_ptr(dev)),
              "gpmpc_linearised_fc_vjp")
    return (gU, gx0) if want_gx0 else gU


def linearised_fc_constraints(means, covs, jac, sc, ds, da):
    """Chance-constraint values and their dense Jacobian on the whole covariance (C ABI ``gpmpc_linearised_fc_constraints``; a pure
    function of a propagated trajectory): g (B, H, m_c) and, when ``jac`` is given, g_jac (B, H m_c, H da)."""
    B, H = means.shape[0], means.shape[1] - 1
    dev = means.device
    out = {"g": _empty(dev, B, H, sc.m)}
    if jac is not None:
        out["g_jac"] = _empty(dev, B, H * sc.m, H * da)
    with torch.cuda.device(dev):
        check(lib().gpmpc_linearised_fc_constraints(B, H, ds, da, ctypes.byref(sc.c), ptr(means), ptr(covs), _vp(jac), ptr(out["g"]),
                                                    _vp(out.get("g_jac")), stream_ptr(dev)), "gpmpc_linearised_fc_constraints")
    return out


def feedback_input_cost(cost, covs, feedback, da, want_dcovs=True):
    """c (B,) = sum_j tr(R K_j Sigma_j K_j^T) over the steps j = 0 ... H-1 of given covariances covs (B, H+1, ds, ds), and with
    ``want_dcovs`` its derivative dcovs (B, H+1, ds, ds) (C ABI ``gpmpc_feedback_input_cost``; a pure function of a trajectory).
    cost: the ``CostParams`` whose R is used; feedback: (da, ds), (H, da, ds) or None (then c = 0)."""
    B, H, ds = covs.shape[0], covs.shape[1] - 1, covs.shape[2]
    dev = covs.device
    K, kstride = _gain(feedback, H, ds, da, dev)
    out = {"c": _empty(dev, B)}
    if want_dcovs:
        out["dcovs"] = _empty(dev, B, H + 1, ds, ds)
    with torch.cuda.device(dev):
        check(lib().gpmpc_feedback_input_cost(B, H, ds, da, ctypes.byref(cost.c), _vp(K), kstride, ptr(covs.contiguous()), ptr(out["c"]),
                                              _vp(out.get("dcovs")), stream_ptr(dev)), "gpmpc_feedback_input_cost")
    return out


def feedback_input_constraints(U, covs, jac, ic, feedback):
    """Input chance-constraint values g_u (B, H, m_u) and, when ``jac`` (B, H, p, p + da) is given, their dense Jacobian g_u_jac
    (B, H m_u, H da) (C ABI ``gpmpc_feedback_input_constraints``; a pure function of a trajectory).  U (B, H, da); covs (B, H+1, ds, ds)."""
    B, H, da = U.shape
    ds = covs.shape[2]
    dev = covs.device
    K, kstride = _gain(feedback, H, ds, da, dev)
    out = {"g_u": _empty(dev, B, H, ic.m)}
    if jac is not None:
        out["g_u_jac"] = _empty(dev, B, H * ic.m, H * da)
    with torch.cuda.device(dev):
        check(lib().gpmpc_feedback_input_constraints(B, H, ds, da, ctypes.byref(ic.c), _vp(K), kstride, ptr(_dev(U, dev)), ptr(covs.contiguous()),
                                                     _vp(jac), ptr(out["g_u"]), _vp(out.get("g_u_jac")), stream_ptr(dev)),
              "gpmpc_feedback_input_constraints")
    return out


def linearised_rollout(model_or_dynamics, x0, U, cost=None, want_grad=True, want_traj=True, want_jac=False, constraints=None, chunk=0,
                       form=None, full_covariance=False, feedback=None, input_cost=False, input_constraints=None):
    """B linearised rollouts (+ cost, gradient, chance constraints) in one call (C ABI ``gpmpc_linearised_rollout``): what ``rollout``
    returns for the same arguments -- cost (B,), grad (B, H, da), means / vars (B, H+1, ds), with ``constraints`` g (B, H, m_c) and g_jac
    (B, H m_c, H da) --, plus ``jac`` (B, H, 2ds, 2ds+da) with ``want_jac`` (which needs ``want_grad``: without it no Jacobian is computed).
    model_or_dynamics: a ``GPModel``, a ``Dynamics`` or a ``SparseDynamics``.  x0 (ds,) or (B, ds); U (H, da) or (B, H, da).
    cost: ``CostParams`` or None (no cost, no grad).  form: see ``linearised_form``.
    full_covariance=True (or a ``feedback`` gain, which implies it): the rule with the whole covariance under u_t = U_t + K_t (x_t - mu_t)
    (C ABI ``gpmpc_linearised_fc_rollout``): ``covs`` (B, H+1, ds, ds) in the place of ``vars``, and ``jac`` is the packed
    (B, H, p, p + da), p = ``packed_dim(ds)``.  feedback: (da, ds) for every step, (H, da, ds), or None.
    input_cost=True / input_constraints (an ``InputConstraints``; either implies the full rule; C ABI ``gpmpc_linearised_fc_rollout_inputs``):
    the commanded input u_t ~ N(U_t, K_t Sigma_t K_t^T) is charged tr(R K_t Sigma_t K_t^T) per step in ``cost`` / ``grad``, and its rows come
    back as ``g_u`` (B, H, m_u) (steps t = 0 ... H-1) and, with ``want_grad``, ``g_u_jac`` (B, H m_u, H da)."""
    _form_code(form)
    model = _model(model_or_dynamics)
    ds, da, dev = model.ds, model.da, model.device
    U = _dev(U, dev)
    if U.dim() == 2:
        U = U[None]
    B, H = U.shape[0], U.shape[1]
    if U.shape[2] != da:
        raise ValueError("U: (H, %d) or (B, H, %d), got %s" % (da, da, tuple(U.shape)))
    U = U.contiguous()
    x0 = _dev(x0, dev).reshape(-1, ds)
    if x0.shape[0] == 1 and B > 1:
        x0 = x0.expand(B, ds).contiguous()
    if x0.shape[0] != B:
        raise ValueError("x0: (%d,) or (%d, %d), got %s" % (ds, B, ds, tuple(x0.shape)))
    if cost is not None and (cost.ds != ds or cost.da != da):
        raise ValueError("shape mismatch between model, x0, U and cost parameters")
    sc = constraints
    if sc is not None and not isinstance(sc, StateConstraints):
        raise TypeError("constraints: a StateConstraints")
    if sc is not None and sc.ds != ds:
        raise ValueError("the constraint rows have %d state coefficients, the model has %d states" % (sc.ds, ds))
    if want_jac and not want_grad:
        raise ValueError("want_jac needs want_grad: without it no Jacobian is computed")
    ic = input_constraints
    if ic is not None and not isinstance(ic, InputConstraints):
        raise TypeError("input_constraints: an InputConstraints")
    if ic is not None and ic.da != da:
        raise ValueError("the input constraint rows have %d coefficients, the model has %d inputs" % (ic.da, da))
    if input_cost and cost is None:
        raise ValueError("input_cost needs a cost: R is the cost's")
    flags = _lib.WANT_GRAD if want_grad else 0
    out = {}
    if cost is not None:
        out["cost"] = _empty(dev, B)
        if want_grad:
            out["grad"] = _empty(dev, B, H, da)
    if sc is not None:
        out["g"] = _empty(dev, B, H, sc.m)
        if want_grad:
            out["g_jac"] = _empty(dev, B, H * sc.m, H * da)
    if full_covariance or feedback is not None or input_cost or ic is not None:
        K, kstride = _gain(feedback, H, ds, da, dev)
        p = packed_dim(ds)
        if want_traj:
            out["means"], out["covs"] = _empty(dev, B, H + 1, ds), _empty(dev, B, H + 1, ds, ds)
        if want_jac:
            out["jac"] = _empty(dev, B, H, p, p + da)
        if input_cost or ic is not None:
            if ic is not None:
                out["g_u"] = _empty(dev, B, H, ic.m)
                if want_grad:
                    out["g_u_jac"] = _empty(dev, B, H * ic.m, H * da)
            icp = ctypes.byref(ic.c) if ic is not None else None
            with torch.cuda.device(dev), linearised_form(form):
                nb = lib().gpmpc_linearised_fc_rollout_inputs_workspace_bytes(ctypes.byref(model.c), B, H, flags, chunk, 1 if input_cost else 0, icp)
                ws = _workspace(dev, nb)
                check(lib().gpmpc_linearised_fc_rollout_inputs(
                    ctypes.byref(model.c), B, H, ptr(x0), _vp(U) if da else None, _vp(K), kstride,
                    ctypes.byref(cost.c) if cost is not None else None, ctypes.byref(sc.c) if sc is not None else None, flags,
                    _vp(out.get("means")), _vp(out.get("covs")), _vp(out.get("jac")), _vp(out.get("cost")), _vp(out.get("grad")),
                    _vp(out.get("g")), _vp(out.get("g_jac")), 1 if input_cost else 0, icp, _vp(out.get("g_u")), _vp(out.get("g_u_jac")), chunk,
                    _vp(ws), nb, stream_ptr(dev)), "gpmpc_linearised_fc_rollout_inputs")
            return out
        with torch.cuda.device(dev), linearised_form(form):
            nb = lib().gpmpc_linearised_fc_rollout_workspace_bytes(ctypes.byref(model.c), B, H, flags, chunk)
            ws = _workspace(dev, nb)
            check(lib().gpmpc_linearised_fc_rollout(ctypes.byref(model.c), B, H, ptr(x0), _vp(U) if da else None, _vp(K), kstride,
                                                    ctypes.byref(cost.c) if cost is not None else None,
                                                    ctypes.byref(sc.c) if sc is not None else None, flags, _vp(out.get("means")),
                                                    _vp(out.get("covs")), _vp(out.get("jac")), _vp(out.get("cost")), _vp(out.get("grad")),
                                                    _vp(out.get("g")), _vp(out.get("g_jac")), chunk, _vp(ws), nb, stream_ptr(dev)),
                  "gpmpc_linearised_fc_rollout")
        return out
    if want_traj:
        out["means"], out["vars"] = _empty(dev, B, H + 1, ds), _empty(dev, B, H + 1, ds)
    if want_jac:
        out["jac"] = _empty(dev, B, H, 2 * ds, 2 * ds + da)
    with torch.cuda.device(dev), linearised_form(form):
        nb = lib().gpmpc_linearised_rollout_workspace_bytes(ctypes.byref(model.c), B, H, flags, chunk)
        ws = _workspace(dev, nb)
        check(lib().gpmpc_linearised_rollout(ctypes.byref(model.c), B, H, ptr(x0), _vp(U) if da else None,
                                             ctypes.byref(cost.c) if cost is not None else None, ctypes.byref(sc.c) if sc is not None else None,
                                             flags, _vp(out.get("means")), _vp(out.get("vars")), _vp(out.get("jac")), _vp(out.get("cost")),
                                             _vp(out.get("grad")), _vp(out.get("g")), _vp(out.get("g_jac")), chunk, _vp(ws), nb, stream_ptr(dev)),
              "gpmpc_linearised_rollout")
    return out                                           # (what the call read stays valid: the caching allocator frees in stream order)


def mppi_solve_linearised(model, x0, U0, cost, constraints=None, samples=64, iterations=30, sigma=1.0, decay=0.9, beta=0.1, seed=0,
                          call_index=0, lb=None, ub=None, form=None, full_covariance=False, feedback=None, input_cost=False,
                          input_constraints=None):
    """``mppi.mppi_solve`` over the linearised rollout (C ABI ``gpmpc_mppi_solve_linearised``): per iteration the sample kernel,
    ``gpmpc_linearised_rollout`` objective only over the K samples (with the constraint values when ``constraints`` is given), the update
    kernel; one device-to-host copy at the end.  Returns what ``mppi_solve`` returns.  form: see ``linearised_form``.
    With ``full_covariance=True`` or a ``feedback`` gain ((da, ds) or (H, da, ds)) the search runs on the full-covariance rule.  That is a
    HOST LOOP, not a single enqueue: per iteration ``mppi_sample``, ``linearised_rollout(..., full_covariance=True, feedback=...)``
    objective only and ``mppi_update`` -- the same kernels, the same sample stream, one launch sequence per iteration from Python.
    ``input_cost`` / ``input_constraints`` (which imply the full rule) are passed on to that rollout; the update sees the state rows followed
    by the input rows, at most 16 together."""
    _form_code(form)
    model = _model(model)
    if full_covariance or feedback is not None or input_cost or input_constraints is not None:
        return _mppi_host_loop_full(model, x0, U0, cost, constraints, samples, iterations, sigma, decay, beta, seed, call_index, lb, ub, form,
                                    feedback, input_cost, input_constraints)
    dev = model.device
    x0, U0 = model_problem(model, x0, U0, cost)
    H, da = U0.shape
    if constraints is not None and constraints.ds != model.ds:
        raise ValueError("the constraint rows have %d state coefficients, the model has %d states" % (constraints.ds, model.ds))
    P = mppi_params(samples, da, sigma, lb, ub, iterations=iterations, decay=decay, beta=beta, seed=seed, call_index=call_index)
    cons = None if constraints is None else ctypes.byref(constraints.c)
    n = H * da
    res = mppi_result_block(n, P.iterations, dev)
    with torch.cuda.device(dev), linearised_form(form):
        nb = lib().gpmpc_mppi_solve_linearised_workspace_bytes(ctypes.byref(model.c), H, ctypes.byref(P), cons)
        ws = _workspace(dev, nb)
        check(lib().gpmpc_mppi_solve_linearised(ctypes.byref(model.c), H, ptr(x0), ptr(U0), ctypes.byref(cost.c), cons, ctypes.byref(P),
                                                ptr(res[:n]), ptr(res[n:n + 2]), ptr(res[n + 2:]), _vp(ws), ws.numel(), stream_ptr(dev)),
              "gpmpc_mppi_solve_linearised")
    return mppi_result(res.cpu().numpy(), H, da)


def _mppi_host_loop_full(model, x0, U0, cost, constraints, samples, iterations, sigma, decay, beta, seed, call_index, lb, ub, form, feedback,
                         input_cost=False, input_constraints=None):
    from .mppi import mppi_sample, mppi_start, mppi_update
    x0, U0 = model_problem(model, x0, U0, cost)
    if iterations < 1:
        raise ValueError("iterations must be at least 1")
    ic = input_constraints
    if ic is not None and (0 if constraints is None else constraints.m) + ic.m > _lib.MAX_CONS:
        raise ValueError("state and input rows together exceed %d" % _lib.MAX_CONS)
    H, da = U0.shape
    mean = U0.contiguous()
    best = mppi_start(mean)
    trace = []
    for it in range(iterations):
        U, x0b = mppi_sample(mean, samples, sigma, lb=lb, ub=ub, seed=seed, call_index=call_index, iteration=it, decay=decay, x0=x0)
        r = linearised_rollout(model, x0b, U, cost, want_grad=False, want_traj=False, constraints=constraints, form=form, full_covariance=True,
                               feedback=feedback, input_cost=input_cost, input_constraints=ic)
        g = r.get("g")
        if ic is not None:
            g = r["g_u"] if g is None else torch.cat([g, r["g_u"]], -1)
        u = mppi_update(U, r["cost"], best, beta, g=g, mean=mean)
        mean, best = u["mean"], u["best"]
        trace.append(u["trace"])
    return mppi_result(torch.cat([best] + trace).cpu().numpy(), H, da, key_first=True)


def lqr_gain(model, x_eq, u_eq, Q, R, iterations=500):
    """A stabilising gain for ``feedback=``: A, B from the mu' rows of ONE linearised step at (x_eq, u_eq) (the device), then the discrete
    Riccati recursion P <- Q + A^T P A - A^T P B (R + B^T P B)^-1 B^T P A in numpy, ``iterations`` times from P = Q.  Returns
    K = -(R + B^T P B)^-1 B^T P A, (da, ds): the sign convention of u = v + K (x - mu)."""
    import numpy as np
    model = _model(model)
    ds, da = model.ds, model.da
    if da < 1:
        raise ValueError("lqr_gain needs action_dim >= 1")
    x_eq = np.asarray(x_eq, dtype=np.float64).reshape(1, ds)
    u_eq = np.asarray(u_eq, dtype=np.float64).reshape(1, da)
    jac = linearised_step(model, x_eq, np.zeros((1, ds)), u_eq, want_jac=True)[2][0].cpu().numpy()
    A, Bm = jac[:ds, :ds], jac[:ds, 2 * ds:]
    return riccati_gain(A, Bm, Q, R, iterations)


def riccati_gain(A, B, Q, R, iterations=500):
    """K = -(R + B^T P B)^-1 B^T P A with P from ``iterations`` steps of the discrete Riccati recursion started at Q (numpy, host)."""
    import numpy as np
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    ds, da = B.shape
    Q = np.asarray(Q, dtype=np.float64).reshape(ds, ds)
    R = np.asarray(R, dtype=np.float64).reshape(da, da)
    P = Q.copy()
    for _ in range(iterations):
        BtP = B.T @ P
        P = Q + A.T @ P @ A - (BtP @ A).T @ np.linalg.solve(R + BtP @ B, BtP @ A)
        P = 0.5 * (P + P.T)
    BtP = B.T @ P
    return -np.linalg.solve(R + BtP @ B, BtP @ A)


__all__ = ["GPModel", "linearised_form", "linearised_step", "linearised_rollout", "mppi_solve_linearised", "linearised_step_full",
           "linearised_fc_vjp", "linearised_fc_constraints", "packed_dim", "lqr_gain", "riccati_gain", "feedback_input_cost",
           "feedback_input_constraints"]
