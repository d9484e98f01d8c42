"""MPPI planner on the device (C ABI ``gpmpc_mppi_*``, kernels in csrc/mppi.hip): K perturbed copies of a plan are
rolled out as one objective-only batch, the plan moves to their softmin-weighted mean, the best sample seen is kept.  With state
constraints a sample is feasible when no row is violated; while none is, the search minimises the total violation.

Plumbing only, like rollout.py: the arithmetic is in the kernels.  ``mppi_sample`` and ``mppi_update`` are the two kernels on their own,
``mppi_solve`` the whole search as one enqueue on the current stream with a single copy of the results at the end.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import MppiParamsC, check, lib, ptr, require_gpu, stream_ptr
from ._solver import mppi_result, mppi_result_block, per_input, solver_problem
from .rollout import _dev, _fullcov_pack

DEFAULTS = {"samples": 64, "iterations": 30, "sigma": None, "decay": 0.9, "beta": 0.1, "seed": 0}


def mppi_params(samples, da, sigma, lb=None, ub=None, iterations=1, decay=1.0, beta=0.1, seed=0, call_index=0):
    """The C struct ``gpmpc_mppi_params``.  sigma, lb, ub: a scalar or one value per input; missing bounds are infinite."""
    if not 1 <= da <= _lib.MAX_D:
        raise ValueError("input dimension exceeds the library limits")
    c = MppiParamsC()
    c.n_samples, c.iterations = int(samples), int(iterations)
    c.sigma[:da] = per_input(sigma, 1.0, da).tolist()
    c.lb[:da] = per_input(lb, -np.inf, da).tolist()
    c.ub[:da] = per_input(ub, np.inf, da).tolist()
    c.sigma_decay, c.beta = float(decay), float(beta)
    c.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c.call_index = int(call_index) & 0xFFFFFFFF
    return c


def mppi_sample(mean, samples, sigma, lb=None, ub=None, seed=0, call_index=0, iteration=0, decay=1.0, x0=None, out=None):
    """``samples`` perturbed copies of the plan ``mean`` (H, da) (C ABI ``gpmpc_mppi_sample``): U (K, H, da), row 0 the plan itself;
    with ``x0`` (ds,) also the start state repeated, (K, ds).  ``out``: a (K, H, da) tensor to write into.  Returns U or (U, x0_batch)."""
    dev = mean.device if isinstance(mean, torch.Tensor) and mean.is_cuda else require_gpu()
    mean = _dev(mean, dev)
    if mean.dim() != 2:
        raise ValueError("mean must have shape (H, da)")
    H, da = mean.shape
    P = mppi_params(samples, da, sigma, lb, ub, decay=decay, seed=seed, call_index=call_index)
    K = P.n_samples
    U = out if out is not None else torch.empty((max(K, 0), H, da), dtype=torch.float64, device=dev)
    if tuple(U.shape) != (K, H, da):
        raise ValueError("out must have shape (samples, H, da)")
    x0d = x0b = None
    ds = 0
    if x0 is not None:
        x0d = _dev(x0, dev).reshape(-1)
        ds = x0d.shape[0]
        x0b = torch.empty((max(K, 0), ds), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().gpmpc_mppi_sample(H, ds, da, ctypes.byref(P), int(iteration), ptr(mean), ptr(x0d), ptr(U), ptr(x0b), stream_ptr()),
              "gpmpc_mppi_sample")
    return U if x0 is None else (U, x0b)


def mppi_start(U0):
    """best = (+inf, +inf, plan): what a search starts from (device tensor (2 + n,))."""
    U0 = U0.reshape(-1)
    return torch.cat((torch.full((2,), float("inf"), dtype=torch.float64, device=U0.device), U0))


def mppi_update(U, cost, best, beta, g=None, mean=None):
    """One update from an evaluated batch (C ABI ``gpmpc_mppi_update``).  U (K, H, da), cost (K,), g (K, H, m_c) or None, best (2 + H da,) =
    (violation, cost, plan) of the best sample so far (``mppi_start``), mean (H, da) the current plan or None: it is returned unchanged
    when no sample is alive (None: NaN then).  Returns dict(mean (H, da), best (2 + n,), trace (6,)): new tensors, the inputs are kept."""
    dev = U.device if isinstance(U, torch.Tensor) and U.is_cuda else require_gpu()
    U, cost, best = _dev(U, dev), _dev(cost, dev).reshape(-1), _dev(best, dev).reshape(-1)
    if U.dim() != 3:
        raise ValueError("U must have shape (K, H, da)")
    K, H, da = U.shape
    n, m_c = H * da, 0
    if g is not None:
        g = _dev(g, dev)
        if g.dim() != 3 or g.shape[0] != K or g.shape[1] != H:
            raise ValueError("g must have shape (K, H, m_c)")
        m_c = g.shape[2]
    if cost.shape[0] != K or best.shape[0] != 2 + n:
        raise ValueError("shape mismatch between U, cost and best")
    new_mean = torch.full((H, da), float("nan"), dtype=torch.float64, device=dev) if mean is None else _dev(mean, dev).reshape(H, da).clone()
    out = {"mean": new_mean, "best": torch.empty_like(best), "trace": torch.empty(6, dtype=torch.float64, device=dev)}
    with torch.cuda.device(dev):
        check(lib().gpmpc_mppi_update(K, H, da, m_c, float(beta), ptr(U), ptr(cost), ptr(g), ptr(out["mean"]), ptr(best), ptr(out["best"]),
                                      ptr(out["trace"]), stream_ptr()), "gpmpc_mppi_update")
    return out


TRACE_FIELDS = ("best_violation", "best_cost", "feasible", "alive", "s_min", "temperature")


def mppi_solve(pack, x0, U0, cost, constraints=None, samples=64, iterations=30, sigma=1.0, decay=0.9, beta=0.1, seed=0, call_index=0,
               lb=None, ub=None, full_covariance=False):
    """The whole search as one enqueue (C ABI ``gpmpc_mppi_solve``): per iteration the sample kernel, ``gpmpc_rollout`` (or
    ``gpmpc_rollout_constrained`` with ``constraints``, a :class:`StateConstraints`) objective-only over the K samples, the update kernel;
    one device-to-host copy at the end.  x0 (ds,), U0 (H, da) the plan the search starts from.
    full_covariance=True: the same search over the full-covariance rollout (C ABI ``gpmpc_mppi_solve_fullcov``:
    ``gpmpc_rollout_fullcov`` / ``gpmpc_rollout_fullcov_constrained``, rows on a^T Sigma_t a).
    Returns dict(U (H, da) numpy: the best plan seen, cost, violation, feasible, trace (iterations, 6) numpy, columns TRACE_FIELDS)."""
    dev = pack.device
    solve, size, what = lib().gpmpc_mppi_solve, lib().gpmpc_mppi_solve_workspace_bytes, "gpmpc_mppi_solve"
    if full_covariance:
        _fullcov_pack(pack)
        solve, size, what = lib().gpmpc_mppi_solve_fullcov, lib().gpmpc_mppi_solve_fullcov_workspace_bytes, "gpmpc_mppi_solve_fullcov"
    x0, U0 = solver_problem(pack, x0, U0, cost, "U0", "(H, da)")
    H, da = U0.shape
    if constraints is not None and constraints.ds != pack.ds:
        raise ValueError("the constraint rows have %d state coefficients, the pack has %d states" % (constraints.ds, pack.ds))
    P = mppi_params(samples, da, sigma, lb, ub, iterations=iterations, decay=decay, beta=beta, seed=seed, call_index=call_index)
    cons = None if constraints is None else ctypes.byref(constraints.c)
    n = H * da
    res = mppi_result_block(n, P.iterations, dev)
    nbytes = size(pack.handle, H, ctypes.byref(P), cons)
    ws = pack.workspace(max(int(nbytes), 256))
    with torch.cuda.device(dev):
        check(solve(pack.handle, H, ptr(x0), ptr(U0), ctypes.byref(cost.c), cons, ctypes.byref(P), ptr(res[:n]),
                    ptr(res[n:n + 2]), ptr(res[n + 2:]), ctypes.c_void_p(ws.data_ptr()), ws.numel(), stream_ptr()), what)
    return mppi_result(res.cpu().numpy(), H, da)
