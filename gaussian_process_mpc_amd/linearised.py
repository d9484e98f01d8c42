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

Plumbing only: the arithmetic is in the kernels.  Every call runs on the current stream of the model's device and returns device tensors."""
import contextlib
import ctypes

import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .mppi import mppi_params
from .particles import GPModel, _dev, _empty, _model, _vp, _workspace
from .rollout import StateConstraints


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


def linearised_rollout(model_or_dynamics, x0, U, cost=None, want_grad=True, want_traj=True, want_jac=False, constraints=None, chunk=0,
                       form=None):
    """B linearised rollouts (+ cost, gradient, chance constraints) in one call (C ABI ``gpmpc_linearised_rollout``): what ``rollout``
    returns for the same arguments -- cost (B,), grad (B, H, da), means / vars (B, H+1, ds), with ``constraints`` g (B, H, m_c) and g_jac
    (B, H m_c, H da) --, plus ``jac`` (B, H, 2ds, 2ds+da) with ``want_jac`` (which needs ``want_grad``: without it no Jacobian is computed).
    model_or_dynamics: a ``GPModel``, a ``Dynamics`` or a ``SparseDynamics``.  x0 (ds,) or (B, ds); U (H, da) or (B, H, da).
    cost: ``CostParams`` or None (no cost, no grad).  form: see ``linearised_form``."""
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
                          call_index=0, lb=None, ub=None, form=None):
    """``mppi.mppi_solve`` over the linearised rollout (C ABI ``gpmpc_mppi_solve_linearised``): per iteration the sample kernel,
    ``gpmpc_linearised_rollout`` objective only over the K samples (with the constraint values when ``constraints`` is given), the update
    kernel; one device-to-host copy at the end.  Returns what ``mppi_solve`` returns.  form: see ``linearised_form``."""
    _form_code(form)
    model = _model(model)
    dev = model.device
    U0 = _dev(U0, dev)
    if U0.dim() != 2 or U0.shape[-1] != model.da:
        raise ValueError("U0 must have shape (H, da)")
    x0 = _dev(x0, dev).reshape(-1)
    if x0.shape[0] != model.ds or cost.ds != model.ds or cost.da != model.da:
        raise ValueError("shape mismatch between model, x0, U0 and cost parameters")
    H, da = U0.shape
    if constraints is not None and constraints.ds != model.ds:
        raise ValueError("the constraint rows have %d state coefficients, the model has %d states" % (constraints.ds, model.ds))
    P = mppi_params(samples, da, sigma, lb, ub, iterations=iterations, decay=decay, beta=beta, seed=seed, call_index=call_index)
    cons = None if constraints is None else ctypes.byref(constraints.c)
    n = H * da
    res = torch.empty(n + 2 + 6 * max(P.iterations, 1), dtype=torch.float64, device=dev)      # [best plan | key | trace]: one block, one copy
    with torch.cuda.device(dev), linearised_form(form):
        nb = lib().gpmpc_mppi_solve_linearised_workspace_bytes(ctypes.byref(model.c), H, ctypes.byref(P), cons)
        ws = _workspace(dev, nb)
        check(lib().gpmpc_mppi_solve_linearised(ctypes.byref(model.c), H, ptr(x0), ptr(U0), ctypes.byref(cost.c), cons, ctypes.byref(P),
                                                ptr(res[:n]), ptr(res[n:n + 2]), ptr(res[n + 2:]), _vp(ws), ws.numel(), stream_ptr(dev)),
              "gpmpc_mppi_solve_linearised")
    host = res.cpu().numpy()
    return {"U": host[:n].reshape(H, da).copy(), "violation": float(host[n]), "cost": float(host[n + 1]), "feasible": bool(host[n] == 0.0),
            "trace": host[n + 2:].reshape(-1, 6).copy()}


__all__ = ["GPModel", "linearised_form", "linearised_step", "linearised_rollout", "mppi_solve_linearised"]
