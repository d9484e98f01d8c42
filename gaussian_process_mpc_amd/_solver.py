"""What the host sides of the device solvers share (mppi.py, device_lbfgs.py, device_auglag.py, and the MPPI solves of linearised.py and
particles.py): per-input parameters, the check of a solve's problem, the result of an MPPI solve, the layout arithmetic of a state
buffer and the chunked enqueue of a search.  Plumbing only."""
import numpy as np
import torch

from .rollout import _dev


def per_input(v, default, da):
    """A scalar or one value per input (None: ``default``) as (da,) float64."""
    return np.broadcast_to(np.asarray(default if v is None else v, dtype=np.float64).reshape(-1), (da,))


def solver_problem(pack, x0, start, cost, name, shape):
    """The start point(s) ``start`` (called ``name``, of shape ``shape``: "(K, H, da)" or "(H, da)") and x0 (ds,) as device tensors, checked
    against the pack and the cost.  Returns (x0, start)."""
    start = _dev(start, pack.device)
    if start.dim() != shape.count(",") + 1 or start.shape[-1] != pack.da:
        raise ValueError("%s must have shape %s" % (name, shape))
    x0 = _dev(x0, pack.device).reshape(-1)
    if x0.shape[0] != pack.ds or cost.ds != pack.ds or cost.da != pack.da:
        raise ValueError("shape mismatch between pack, x0, %s and cost parameters" % name)
    return x0, start


def model_problem(model, x0, U0, cost):
    """``solver_problem`` for the MPPI solves that take a ``GPModel`` in the place of a pack: (x0 (ds,), U0 (H, da)) on the model's device."""
    U0 = _dev(U0, model.device)
    if U0.dim() != 2 or U0.shape[-1] != model.da:
        raise ValueError("U0 must have shape (H, da)")
    x0 = _dev(x0, model.device).reshape(-1)
    if x0.shape[0] != model.ds or cost.ds != model.ds or cost.da != model.da:
        raise ValueError("shape mismatch between model, x0, U0 and cost parameters")
    return x0, U0


def mppi_result_block(n, iterations, dev):
    """The device block an MPPI solve writes, [best plan (n) | key (2) | trace (6 per iteration)]: one block, one copy at the end."""
    return torch.empty(n + 2 + 6 * max(iterations, 1), dtype=torch.float64, device=dev)


def mppi_result(host, H, da, key_first=False):
    """What every MPPI solve returns, from the host copy of its block (``key_first``: [key | best plan | trace], a host loop's)."""
    n = H * da
    plan, key = (host[2:2 + n], host[:2]) if key_first else (host[:n], host[n:n + 2])
    return {"U": plan.reshape(H, da).copy(), "violation": float(key[0]), "cost": float(key[1]), "feasible": bool(key[0] == 0.0),
            "trace": host[n + 2:].reshape(-1, 6).copy()}


def state_layout(sizes):
    """Offsets (in doubles) of the fields [(name, doubles), ...] of a state buffer, each field rounded up to 32 doubles, and ``total``: the
    arithmetic of include/gpmpc.h."""
    L, o = {}, 0
    for name, size in sizes:
        L[name] = o
        o += (size + 31) & ~31
    L["total"] = o
    return L


def enqueue_chunks(budget, every, enqueue, ws, after=None):
    """A search of ``budget`` steps as enqueues of ``every`` steps (0: one chunk of ``budget``): ``enqueue(first, count)``, then
    ``after(done)`` (optional), then ONE read of ws[0] -- the count of starts still searching --, until that is 0 or the budget is spent.
    At least one enqueue is made; a negative budget is passed on as it is (the library's to refuse).  Returns (done, enqueues)."""
    chunk = every if every > 0 else max(budget, 0)
    done = calls = 0
    while True:
        count = budget if budget < 0 else min(chunk, budget - done)
        enqueue(done, count)
        done += count
        calls += 1
        if after is not None:
            after(done)
        if done >= budget or ws[0].item() == 0.0:
            return done, calls
