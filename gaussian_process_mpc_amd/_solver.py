"""What the host sides of the device solvers share (mppi.py, device_lbfgs.py, device_auglag.py): per-input parameters, the check of a
solve's problem, the layout arithmetic of a state buffer and the chunked enqueue of a search.  Plumbing only."""
import numpy as np

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
