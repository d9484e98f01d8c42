"""Lock-step multi-start L-BFGS on the device (C ABI ``gpmpc_lbfgs_*``, kernels in csrc/lbfgs.hip): the rule of
``multistart.lockstep_lbfgs`` (``line_points=1``, no ``patience``) with the state machine of every start in one small kernel between two
batched rollouts, so that a tick needs neither a device-to-host copy nor the host.

Plumbing only, like mppi.py: the arithmetic is in the kernels.  ``lbfgs_start`` and ``lbfgs_tick`` are the pure entries over a state buffer
(one tensor of doubles, layout in include/gpmpc.h, viewed field by field with ``lbfgs_state_view``); ``lbfgs_solve`` is the whole search,
enqueued in chunks of ``check_every`` ticks on the current stream with one read of the not-done counter per chunk.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import LbfgsParamsC, check, lib, ptr, require_gpu, stream_ptr
from ._solver import enqueue_chunks, per_input, solver_problem, state_layout
from .rollout import _dev, _fullcov_pack

SCALARS = ("F", "converged", "alive", "iters", "ticks", "done", "A", "cnt", "head")


def lbfgs_params(n_starts, da, lb=None, ub=None, history=8, gtol=1e-4, ftol=1e-10, c1=1e-4, min_step=1e-12):
    """The C struct ``gpmpc_lbfgs_params``.  lb, ub: a scalar or one value per input; missing bounds are infinite."""
    if not 1 <= da <= _lib.MAX_D:
        raise ValueError("input dimension exceeds the library limits")
    c = LbfgsParamsC()
    c.n_starts, c.history = int(n_starts), int(history)
    c.gtol, c.ftol, c.c1, c.min_step = float(gtol), float(ftol), float(c1), float(min_step)
    c.lb[:da] = per_input(lb, -np.inf, da).tolist()
    c.ub[:da] = per_input(ub, np.inf, da).tolist()
    return c


def lbfgs_state_layout(K, n, m):
    """Offsets (in doubles) of every field of the state buffer, and ``total``: the arithmetic of include/gpmpc.h."""
    return state_layout([("summary", 32), ("plan", n)] + [(f, K) for f in SCALARS] + [("rho", K * m)]
                        + [(f, K * n) for f in ("X", "G", "D", "U")] + [(f, K * m * n) for f in ("S", "Y")])


def lbfgs_state_view(state, K, H, da, m):
    """Every field of a state buffer as a view of it (no copy): summary (32,), plan (H, da), the per-start scalars (K,), rho (K, m),
    X, G, D (K, n), U (K, H, da), S, Y (K, m, n) -- rho, S and Y by ring SLOT (pair j, 0 = newest, is in slot (head + j) mod m)."""
    n = H * da
    L = lbfgs_state_layout(K, n, m)
    if state.numel() < L["total"]:
        raise ValueError("the state buffer is smaller than its layout")
    v = {"summary": state[:32], "plan": state[L["plan"]:L["plan"] + n].view(H, da)}
    for f in SCALARS:
        v[f] = state[L[f]:L[f] + K]
    v["rho"] = state[L["rho"]:L["rho"] + K * m].view(K, m)
    for f in ("X", "G", "D"):
        v[f] = state[L[f]:L[f] + K * n].view(K, n)
    v["U"] = state[L["U"]:L["U"] + K * n].view(K, H, da)
    for f in ("S", "Y"):
        v[f] = state[L[f]:L[f] + K * m * n].view(K, m, n)
    return v


def lbfgs_state_fields(state, K, H, da, m):
    """The state as numpy arrays in the terms of the rule: rho (K, m), S, Y (K, m, n) NEWEST FIRST (the ring unrolled; slots past cnt as they
    are), XT (K, n) the trial points, flags as bool, counters as int64, plus not_done, best, f_best of the summary."""
    host = state.detach().cpu().numpy()
    v = lbfgs_state_view(torch.from_numpy(host), K, H, da, m)
    out = {f: v[f].numpy().copy() for f in ("F", "A", "X", "G", "D")}
    for f in ("converged", "alive", "done"):
        out[f] = v[f].numpy() != 0.0
    for f in ("iters", "ticks", "cnt", "head"):
        out[f] = v[f].numpy().astype(np.int64)
    order = (out["head"][:, None] + np.arange(m)[None, :]) % m
    rows = np.arange(K)[:, None]
    out["rho"] = v["rho"].numpy()[rows, order]
    out["S"], out["Y"] = v["S"].numpy()[rows, order], v["Y"].numpy()[rows, order]
    out["XT"] = v["U"].numpy().reshape(K, -1).copy()
    s = v["summary"].numpy()
    out["not_done"], out["best"], out["f_best"] = int(s[0]), int(s[1]), float(s[2])
    out["plan"] = v["plan"].numpy().reshape(-1).copy()
    return out


def lbfgs_state_from_fields(fields, H, da, device=None):
    """A state buffer (device tensor of doubles) from arrays in the terms of the rule -- the inverse of ``lbfgs_state_fields``: rho, S, Y
    newest first, placed in the ring from ``fields["head"]`` (K,) on (default 0: the newest pair in slot 0); the summary and the plan are
    left zero (the next tick writes them)."""
    dev = require_gpu() if device is None else device
    S = np.asarray(fields["S"], dtype=np.float64)
    K, m, n = S.shape
    head = np.asarray(fields.get("head", np.zeros(K)), dtype=np.int64).reshape(K)
    slot = (head[:, None] + np.arange(m)[None, :]) % m          # pair j of start k lives in slot[k, j]
    rows = np.arange(K)[:, None]
    ring = {}
    for f in ("rho", "S", "Y"):
        a = np.asarray(fields[f], dtype=np.float64)
        ring[f] = np.empty_like(a)
        ring[f][rows, slot] = a
    host = torch.zeros(lbfgs_state_layout(K, n, m)["total"], dtype=torch.float64)
    v = lbfgs_state_view(host, K, H, da, m)
    for f in ("F", "A", "X", "G", "D", "converged", "alive", "done", "iters", "cnt"):
        v[f].copy_(torch.from_numpy(np.asarray(fields[f], dtype=np.float64).reshape(tuple(v[f].shape))))
    for f in ("rho", "S", "Y"):
        v[f].copy_(torch.from_numpy(ring[f]))
    v["head"].copy_(torch.from_numpy(head.astype(np.float64)))
    v["ticks"].copy_(torch.from_numpy(np.asarray(fields.get("ticks", np.zeros(K)), dtype=np.float64)))
    v["U"].copy_(torch.from_numpy(np.asarray(fields["XT"], dtype=np.float64).reshape(K, H, da)))
    return host.to(dev)


def lbfgs_start(X0, cost=None, grad=None, lb=None, ub=None, history=8, gtol=1e-4, ftol=1e-10, c1=1e-4, min_step=1e-12, x0=None, state=None):
    """The start step (C ABI ``gpmpc_lbfgs_start``).  X0 (K, H, da); cost (K,), grad (K, H, da): the evaluation of clip(X0).  With cost and
    grad None only U = clip(X0) is written: the batch that evaluation runs on.  ``state``: the buffer to write into (a new one otherwise).
    With ``x0`` (ds,) also returns the start state repeated, (K, ds).  Returns state or (state, x0_batch)."""
    dev = X0.device if isinstance(X0, torch.Tensor) and X0.is_cuda else require_gpu()
    X0 = _dev(X0, dev)
    if X0.dim() != 3:
        raise ValueError("X0 must have shape (K, H, da)")
    K, H, da = X0.shape
    P = lbfgs_params(K, da, lb, ub, history, gtol, ftol, c1, min_step)
    if (cost is None) != (grad is None):
        raise ValueError("cost and grad are given together")
    if cost is not None:
        cost, grad = _dev(cost, dev).reshape(-1), _dev(grad, dev).reshape(K, -1)
        if cost.shape[0] != K or grad.shape[1] != H * da:
            raise ValueError("shape mismatch between X0, cost and grad")
    if state is None:
        nbytes = lib().gpmpc_lbfgs_state_bytes(K, H, da, P.history)
        state = torch.zeros(max(int(nbytes) // 8, 32), dtype=torch.float64, device=dev)
    x0d = x0b = None
    ds = 0
    if x0 is not None:
        x0d = _dev(x0, dev).reshape(-1)
        ds = x0d.shape[0]
        x0b = torch.empty((K, ds), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().gpmpc_lbfgs_start(H, ds, da, ctypes.byref(P), ptr(X0), ptr(cost), ptr(grad), ptr(x0d), ptr(x0b), ptr(state),
                                      state.numel() * 8, stream_ptr()), "gpmpc_lbfgs_start")
    return state if x0 is None else (state, x0b)


def lbfgs_tick(state, cost, grad, K, H, da, lb=None, ub=None, history=8, gtol=1e-4, ftol=1e-10, c1=1e-4, min_step=1e-12,
               full_covariance=False):
    """One tick, in place (C ABI ``gpmpc_lbfgs_tick``): cost (K,), grad (K, H, da) the evaluation of the state's U.  Returns ``state``.
    full_covariance: accepted so that a chain of ticks takes the keywords of ``lbfgs_solve``; not consulted -- the tick is a pure function
    of (cost, grad), whichever rollout (``rollout`` or ``rollout_fullcov``) the caller evaluated them with."""
    dev = state.device
    P = lbfgs_params(K, da, lb, ub, history, gtol, ftol, c1, min_step)
    cost, grad = _dev(cost, dev).reshape(-1), _dev(grad, dev).reshape(K, -1)
    if cost.shape[0] != K or grad.shape[1] != H * da:
        raise ValueError("shape mismatch between the state, cost and grad")
    with torch.cuda.device(dev):
        check(lib().gpmpc_lbfgs_tick(H, da, ctypes.byref(P), ptr(cost), ptr(grad), ptr(state), state.numel() * 8, stream_ptr()),
              "gpmpc_lbfgs_tick")
    return state


def lbfgs_solve(pack, x0, X0, cost, lb=None, ub=None, max_ticks=150, history=8, gtol=1e-4, ftol=1e-10, check_every=8, c1=1e-4,
                min_step=1e-12, callback=None, full_covariance=False):
    """The whole search (C ABI ``gpmpc_lbfgs_solve``; full_covariance=True: ``gpmpc_lbfgs_solve_fullcov``, the same search with
    ``gpmpc_rollout_fullcov`` as its evaluation): ``check_every`` ticks per enqueue -- each tick ``gpmpc_rollout`` with gradient over the K
    trial points and the tick kernel, no host synchronisation in between --, then one read of the not-done counter; it stops when that is 0
    or ``max_ticks`` is reached.  ``check_every=0``: one chunk of ``max_ticks``.  x0 (ds,), X0 (K, H, da) the start points.
    ``callback(ticks_enqueued, state)`` (optional) is called after every chunk with the state buffer (``lbfgs_state_view``).
    Returns (U (H, da) numpy: the best plan, its cost, info) with the keys of ``multistart.lockstep_lbfgs``'s info."""
    dev = pack.device
    solve, size, what = lib().gpmpc_lbfgs_solve, lib().gpmpc_lbfgs_solve_workspace_bytes, "gpmpc_lbfgs_solve"
    if full_covariance:
        _fullcov_pack(pack)
        solve, size, what = lib().gpmpc_lbfgs_solve_fullcov, lib().gpmpc_lbfgs_solve_fullcov_workspace_bytes, "gpmpc_lbfgs_solve_fullcov"
    x0, X0 = solver_problem(pack, x0, X0, cost, "X0", "(K, H, da)")
    K, H, da = X0.shape
    n = H * da
    max_ticks, check_every = int(max_ticks), int(check_every)
    if check_every < 0:
        raise ValueError("check_every must be 0 (one chunk) or positive")
    P = lbfgs_params(K, da, lb, ub, history, gtol, ftol, c1, min_step)
    nbytes = int(size(pack.handle, H, ctypes.byref(P)))
    # a buffer of the search's own: the state lives in it between the chunks (the pack's per-stream scratch is anybody's between two calls)
    ws = torch.empty(max(nbytes // 8, 32), dtype=torch.float64, device=dev)
    L = lbfgs_state_layout(K, n, P.history)
    ws[:L["total"]].zero_()                                  # (the padding between the fields is never written by a kernel)

    def enqueue(first_tick, n_ticks):
        check(solve(pack.handle, H, ptr(x0), ptr(X0), ctypes.byref(cost.c), ctypes.byref(P), first_tick, n_ticks,
                    ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, stream_ptr()), what)

    with torch.cuda.device(dev):
        done_ticks, _ = enqueue_chunks(max_ticks, check_every, enqueue, ws, None if callback is None else lambda done: callback(done, ws))
    host = ws[:L["G"]].cpu().numpy()                                      # one copy: everything before G is what a caller reads
    col = lambda f: host[L[f]:L[f] + K]                                   # noqa: E731
    ticks = int(col("ticks").max())
    info = {"f": col("F").copy(), "x": host[L["X"]:L["X"] + K * n].reshape(K, n).copy(), "ticks": ticks, "evaluations": ticks + 1,
            "converged": col("converged") != 0.0, "alive": col("alive") != 0.0, "best": int(host[1]),
            "iterations": col("iters").astype(np.int64), "ticks_enqueued": done_ticks}
    return host[L["plan"]:L["plan"] + n].reshape(H, da).copy(), float(host[2]), info
