"""Constrained multi-start on the device (C ABI ``gpmpc_auglag_*``, kernels in csrc/auglag.hip): an augmented
Lagrangian over ``gpmpc_rollout_constrained`` with the lock-step L-BFGS of device_lbfgs.py as the inner search -- K constrained searches
advanced together, multipliers and penalties updated on the device between the inner searches.

Plumbing only, like device_lbfgs.py: the arithmetic is in the kernels.  ``auglag_merit`` and ``auglag_outer`` are the pure entries
(``auglag_outer`` over a state buffer: one tensor of doubles, layout in include/gpmpc.h, viewed field by field with ``auglag_state_view``);
``auglag_solve`` is the whole solve, enqueued in chunks of ``check_outer`` outer iterations on the current stream with one read of the
not-settled counter per chunk.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import AuglagParamsC, check, lib, ptr, require_gpu, stream_ptr
from .device_lbfgs import lbfgs_params, lbfgs_state_layout
from ._solver import enqueue_chunks, per_input, solver_problem, state_layout
from .rollout import _dev, _fullcov_pack

SCALARS = ("rho", "V_prev", "v", "f", "inc_v", "inc_f", "alive", "settled")


def auglag_params(n_starts, da, lb=None, ub=None, inner_ticks=25, rho0=10.0, growth=10.0, shrink=0.25, rho_max=1e8, lam_max=1e12,
                  feas_tol=1e-4, history=8, gtol=1e-6, ftol=1e-12, c1=1e-4, min_step=1e-12):
    """The C struct ``gpmpc_auglag_params``: the inner search's ``gpmpc_lbfgs_params`` (``lbfgs_params``) and the outer rule's scalars."""
    c = AuglagParamsC()
    c.inner = lbfgs_params(n_starts, da, lb, ub, history, gtol, ftol, c1, min_step)
    c.rho0, c.growth, c.shrink, c.rho_max = float(rho0), float(growth), float(shrink), float(rho_max)
    c.lam_max, c.feas_tol, c.inner_ticks = float(lam_max), float(feas_tol), int(inner_ticks)
    return c


def auglag_state_layout(K, n, R):
    """Offsets (in doubles) of every field of the state buffer, and ``total``: the arithmetic of include/gpmpc.h."""
    return state_layout([("summary", 32), ("plan", n)] + [(f, K) for f in SCALARS] + [("lam", K * R), ("inc_x", K * n)])


def auglag_state_view(state, K, H, da, m_c):
    """Every field of a state buffer as a view of it (no copy): summary (32,), plan (H, da), the per-start scalars (K,), lam (K, H m_c),
    inc_x (K, H da)."""
    n, R = H * da, H * m_c
    L = auglag_state_layout(K, n, R)
    if state.numel() < L["total"]:
        raise ValueError("the state buffer is smaller than its layout")
    v = {"summary": state[:32], "plan": state[L["plan"]:L["plan"] + n].view(H, da)}
    for f in SCALARS:
        v[f] = state[L[f]:L[f] + K]
    v["lam"] = state[L["lam"]:L["lam"] + K * R].view(K, R)
    v["inc_x"] = state[L["inc_x"]:L["inc_x"] + K * n].view(K, n)
    return v


def auglag_state_fields(state, K, H, da, m_c):
    """The state as numpy arrays in the terms of the rule: floats as they are, alive and settled as bool, plus not_settled, best and the
    best key (best_v, best_f) of the summary."""
    host = state[:auglag_state_layout(K, H * da, H * m_c)["total"]].detach().cpu().numpy()
    v = auglag_state_view(torch.from_numpy(host), K, H, da, m_c)
    out = {f: v[f].numpy().copy() for f in ("rho", "V_prev", "v", "f", "inc_v", "inc_f", "lam", "inc_x")}
    for f in ("alive", "settled"):
        out[f] = v[f].numpy() != 0.0
    s = v["summary"].numpy()
    out["not_settled"], out["best"], out["best_v"], out["best_f"] = int(s[0]), int(s[1]), float(s[2]), float(s[3])
    out["plan"] = v["plan"].numpy().reshape(-1).copy()
    return out


def auglag_state_new(X0, rho0, m_c, lb=None, ub=None):
    """The state a solve starts from, for a caller that drives the outer steps itself: rho = rho0, lam = 0, V_prev, v, f and the incumbent
    keys +inf, the incumbent plans clip(X0), alive, not settled; the summary and the plan are left zero (the next outer step writes them).
    X0 (K, H, da) on the device."""
    K, H, da = X0.shape
    state = torch.zeros(auglag_state_layout(K, H * da, H * m_c)["total"], dtype=torch.float64, device=X0.device)
    v = auglag_state_view(state, K, H, da, m_c)
    bound = lambda b, d: torch.as_tensor(per_input(b, d, da).copy(), device=X0.device)  # noqa: E731
    v["inc_x"].copy_(torch.minimum(torch.maximum(X0, bound(lb, -np.inf)), bound(ub, np.inf)).reshape(K, -1))
    v["rho"].fill_(float(rho0))
    for f in ("V_prev", "v", "f", "inc_v", "inc_f"):
        v[f].fill_(float("inf"))
    v["alive"].fill_(1.0)
    return state


def auglag_merit(f, grad, g, g_jac, lam, rho):
    """Merit value and gradient (C ABI ``gpmpc_auglag_merit``).  f (K,), grad (K, H, da), g (K, H, m_c), g_jac (K, H m_c, H da) as
    ``rollout(..., constraints=)`` returns them; lam (K, H m_c), rho (K,).  Returns (M (K,), dM (K, H, da))."""
    dev = grad.device if isinstance(grad, torch.Tensor) and grad.is_cuda else require_gpu()
    grad, g = _dev(grad, dev), _dev(g, dev)
    if grad.dim() != 3 or g.dim() != 3 or g.shape[:2] != grad.shape[:2]:
        raise ValueError("grad must have shape (K, H, da) and g (K, H, m_c)")
    K, H, da = grad.shape
    m_c = g.shape[2]
    n, R = H * da, H * m_c
    f, g_jac, lam, rho = _dev(f, dev).reshape(-1), _dev(g_jac, dev), _dev(lam, dev), _dev(rho, dev).reshape(-1)
    if f.shape[0] != K or rho.shape[0] != K or g_jac.numel() != K * R * n or lam.numel() != K * R:
        raise ValueError("shape mismatch between f, grad, g, g_jac, lam and rho")
    M = torch.empty(K, dtype=torch.float64, device=dev)
    dM = torch.empty((K, H, da), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().gpmpc_auglag_merit(K, H, da, m_c, ptr(f), ptr(grad), ptr(g), ptr(g_jac), ptr(lam), ptr(rho), ptr(M), ptr(dM), stream_ptr()),
              "gpmpc_auglag_merit")
    return M, dM


def auglag_outer(state, f, g, X, K, H, da, update=True, conv=None, alive=None, params=None, **options):
    """One outer step of every start, in place (C ABI ``gpmpc_auglag_outer``): f (K,), g (K, H, m_c) the evaluation of the points X
    (K, H, da); conv, alive (K,) or None: the inner search's flags.  ``params``: an ``auglag_params`` struct, or its keyword options.
    Returns ``state``."""
    dev = state.device
    g = _dev(g, dev)
    if g.dim() != 3 or g.shape[0] != K or g.shape[1] != H:
        raise ValueError("g must have shape (K, H, m_c)")
    m_c = g.shape[2]
    P = params if params is not None else auglag_params(K, da, **options)
    f, X = _dev(f, dev).reshape(-1), _dev(X, dev).reshape(K, -1)
    conv = None if conv is None else _dev(conv, dev).reshape(-1)
    alive = None if alive is None else _dev(alive, dev).reshape(-1)
    if f.shape[0] != K or X.shape[1] != H * da or any(a is not None and a.shape[0] != K for a in (conv, alive)):
        raise ValueError("shape mismatch between the state, f, g and X")
    with torch.cuda.device(dev):
        check(lib().gpmpc_auglag_outer(H, da, m_c, ctypes.byref(P), int(bool(update)), ptr(f), ptr(g), ptr(X), ptr(conv), ptr(alive),
                                       ptr(state), state.numel() * 8, stream_ptr()), "gpmpc_auglag_outer")
    return state


def auglag_solve(pack, x0, X0, cost, constraints, lb=None, ub=None, outer=8, inner_ticks=25, rho0=10.0, growth=10.0, shrink=0.25,
                 rho_max=1e8, lam_max=1e12, feas_tol=1e-4, history=8, gtol=1e-6, ftol=1e-12, check_outer=1, callback=None, c1=1e-4,
                 min_step=1e-12, full_covariance=False):
    """The whole solve (C ABI ``gpmpc_auglag_solve``; full_covariance=True: ``gpmpc_auglag_solve_fullcov``, the same solve with
    ``gpmpc_rollout_fullcov_constrained`` as its evaluation, rows on a^T Sigma_t a): ``check_outer`` outer iterations per enqueue -- each one constrained evaluation, the
    outer step, the restart of the inner search and ``inner_ticks`` x (constrained rollout with gradient, merit kernel, tick kernel), no
    host synchronisation in between --, then one read of the count of alive starts that are not settled; it stops when that is 0 or
    ``outer`` is reached.  ``check_outer=0``: one chunk of ``outer``.  x0 (ds,), X0 (K, H, da) the start points, ``constraints`` a
    :class:`StateConstraints`.  ``callback(outer_done, workspace, inner_offset)`` (optional) is called after every chunk: the workspace
    begins with the state (``auglag_state_view``), the inner search's state (``lbfgs_state_view``) begins ``inner_offset`` doubles in.
    Returns (U (H, da) numpy: the incumbent of the best start, its cost, info): info holds per start f and violation (the incumbent's cost and
    max(g, 0), 0 where feasible), feasible, x (the incumbents), rho, lam, alive, settled, and best, outer, evaluations."""
    dev = pack.device
    solve, size, what = lib().gpmpc_auglag_solve, lib().gpmpc_auglag_solve_workspace_bytes, "gpmpc_auglag_solve"
    if full_covariance:
        _fullcov_pack(pack)
        solve, size, what = lib().gpmpc_auglag_solve_fullcov, lib().gpmpc_auglag_solve_fullcov_workspace_bytes, "gpmpc_auglag_solve_fullcov"
    x0, X0 = solver_problem(pack, x0, X0, cost, "X0", "(K, H, da)")
    K, H, da = X0.shape
    n = H * da
    if constraints is None:
        raise ValueError("auglag_solve needs state constraints: the unconstrained multi-start is device_lbfgs.lbfgs_solve")
    if constraints.ds != pack.ds:
        raise ValueError("constraint rows must have one coefficient per state dimension")
    outer, check_outer = int(outer), int(check_outer)
    if check_outer < 0:
        raise ValueError("check_outer must be 0 (one chunk) or positive")
    m_c = constraints.m
    R = H * m_c
    P = auglag_params(K, da, lb, ub, inner_ticks, rho0, growth, shrink, rho_max, lam_max, feas_tol, history, gtol, ftol, c1, min_step)
    nbytes = int(size(pack.handle, H, ctypes.byref(constraints.c), ctypes.byref(P)))
    # a buffer of the solve's own: both states live in it between the chunks
    ws = torch.empty(max(nbytes // 8, 32), dtype=torch.float64, device=dev)
    L = auglag_state_layout(K, n, R)
    inner_total = lbfgs_state_layout(K, n, P.inner.history)["total"] if 1 <= P.inner.history <= _lib.LBFGS_MAX_HISTORY else 0
    ws[:min(L["total"] + inner_total, ws.numel())].zero_()    # (the padding between the fields is never written by a kernel)

    def enqueue(first_outer, n_outer):
        check(solve(pack.handle, H, ptr(x0), ptr(X0), ctypes.byref(cost.c), ctypes.byref(constraints.c),
                    ctypes.byref(P), first_outer, n_outer, ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), what)

    with torch.cuda.device(dev):
        done, calls = enqueue_chunks(outer, check_outer, enqueue, ws, None if callback is None else lambda d: callback(d, ws, L["total"]))
    s = auglag_state_fields(ws, K, H, da, m_c)
    info = {"f": s["inc_f"], "violation": s["inc_v"], "feasible": s["inc_v"] == 0.0, "x": s["inc_x"], "best": s["best"], "rho": s["rho"],
            "lam": s["lam"], "outer": done, "evaluations": done * (1 + int(inner_ticks)) + calls, "settled": s["settled"], "alive": s["alive"],
            "last_f": s["f"], "last_violation": s["v"]}
    return s["plan"].reshape(H, da), float(s["best_f"]), info
