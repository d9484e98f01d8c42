"""numpy restatement of the MPPI planner, for tests/test_host_mppi.py and tests/test_gpu_mppi.py.

Written from the specification in include/gpmpc.h, sharing no code with csrc/mppi.hip:

* ``philox4x32_10``: the counter-based generator of Salmon et al. (SC'11), vectorised over counters;
* ``normals``: the 53-bit uniforms and Box-Muller of the header, element e of stream (seed, call index, iteration);
* ``sample``: U[k][c] = clamp(mean[c] + sigma_j decay^it eps[k][c], lb_j, ub_j), row 0 the mean itself;
* ``update``: liveness, violation, scores, argmin, best key, temperature, weights, weighted mean -- with the summation orders the header's
  "fixed order" leaves to the implementation and csrc/mppi.hip documents (sequential violation; 256 strided partial sums folded in
  halves), so that the trace can be compared exactly;
* ``solve``: the loop over ``oracle.forward_propagate(..., "o2")`` + ``oracle.cost``.
"""
import numpy as np
import torch

from oracle import gpmpc_oracle as O

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
TWO_PI = 2.0 * np.pi


def philox4x32_10(counter, key):
    """counter: (..., 4) integers < 2^32, key: (2,) integers < 2^32 -> (..., 4) uint64 holding 32-bit words."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]), int(key[1])
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
    return np.stack(c, axis=-1)


def _uniform(hi, lo):
    return ((hi >> np.uint64(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint64(6)).astype(np.float64) + 0.5) * 2.0 ** -53


def normals(seed, call_index, iteration, count):
    """eps[e], e < count, of the stream (seed, call_index, iteration)."""
    pairs = (count + 1) // 2
    p = np.arange(pairs, dtype=np.uint64)
    ctr = np.stack((p & MASK, p >> np.uint64(32), np.full(pairs, iteration, dtype=np.uint64), np.full(pairs, call_index, dtype=np.uint64)), axis=-1)
    w = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u1, u2 = _uniform(w[:, 0], w[:, 1]), _uniform(w[:, 2], w[:, 3])
    assert np.all((u1 > 0) & (u2 > 0))
    r = np.sqrt(-2.0 * np.log(u1))
    eps = np.empty(2 * pairs)
    eps[0::2] = r * np.cos(TWO_PI * u2)
    eps[1::2] = r * np.sin(TWO_PI * u2)
    return eps[:count]


def sample(mean, K, da, sigma, lb, ub, seed=0, call_index=0, iteration=0, decay=1.0):
    """(K, n) samples around mean (n,); sigma, lb, ub: (da,)."""
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)
    n = mean.size
    j = np.arange(n) % da
    sg, lo, hi = (np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(-1), (da,))[j] for v in (sigma, lb, ub))
    eps = normals(seed, call_index, iteration, K * n).reshape(K, n)
    U = np.minimum(np.maximum(mean[None, :] + (sg * decay ** iteration)[None, :] * eps, lo[None, :]), hi[None, :])
    U[0] = mean
    return U


def _fold(terms):
    """Sum of terms[k], k ascending within each of 256 strided partial sums, the partial sums folded in halves."""
    terms = np.asarray(terms, dtype=np.float64)
    pad = np.zeros((-terms.size) % 256)
    rows = np.concatenate((terms, pad)).reshape(-1, 256)
    p = np.zeros(256)
    for row in rows:
        p = p + row
    h = 128
    while h >= 1:
        p = p[:h] + p[h:2 * h]
        h //= 2
    return float(p[0])


def update(U, cost, g, mean, best, beta):
    """U (K, n), cost (K,), g (K, m) or None, mean (n,), best (2 + n,) -> dict(mean, best, trace (6,), kstar, weights)."""
    U, cost = np.asarray(U, dtype=np.float64), np.asarray(cost, dtype=np.float64)
    K, n = U.shape
    best = np.asarray(best, dtype=np.float64).copy()
    dead = np.isnan(cost)
    v = np.zeros(K)
    if g is not None:
        g = np.asarray(g, dtype=np.float64).reshape(K, -1)
        dead = dead | np.isnan(g).any(axis=1)
        for i in range(g.shape[1]):
            v = v + np.where(g[:, i] > 0.0, g[:, i], 0.0)
    alive = ~dead
    feas = alive & (v == 0.0)
    if not alive.any():
        return {"mean": np.asarray(mean, dtype=np.float64).copy(), "best": best,
                "trace": np.array([best[0], best[1], 0.0, 0.0, np.inf, 0.0]), "kstar": None, "weights": np.zeros(K)}
    restore = not feas.any()
    cand = alive if restore else feas
    s = np.where(cand, v if restore else cost, np.inf)
    idx = np.flatnonzero(cand)
    kstar = int(idx[np.argmin(s[idx])])                      # (argmin returns the first of equal minima)
    smin = s[kstar]
    key = (smin if restore else 0.0, cost[kstar])
    if key[0] < best[0] or (key[0] == best[0] and key[1] < best[1]):
        best[0], best[1] = key
        best[2:] = U[kstar]
    fin = cand & np.isfinite(s)
    nfin = int(fin.sum())
    T = beta * (_fold(np.where(fin, s, 0.0)) / float(nfin) - smin) if nfin else 0.0
    if T > 0.0 and T < np.inf:
        with np.errstate(invalid="ignore", over="ignore"):
            w = np.where(fin, np.exp(-(np.where(fin, s, smin) - smin) / T), 0.0)
    else:
        w = np.where(cand & (s == smin), 1.0, 0.0)
    new_mean = (w[:, None] * U)[w != 0.0].sum(axis=0) / w.sum()
    return {"mean": new_mean, "best": best, "trace": np.array([best[0], best[1], float(feas.sum()), float(alive.sum()), smin, T]),
            "kstar": kstar, "weights": w}


def oracle_evaluate(gp, H, x0, pb, gamma, rows=None):
    """U (K, n) -> (cost (K,), g (K, H m_c) or None) by the pinned oracle, one plan at a time."""
    from constraints_reference import g_of_trajectory

    def evaluate(U):
        cost, g = [], []
        for u in U:
            Ut = torch.as_tensor(u.reshape(H, -1))
            means, covs = O.forward_propagate(gp, H, torch.as_tensor(np.asarray(x0, dtype=np.float64)), Ut, "o2")
            cost.append(float(O.cost(means, Ut, covs, torch.as_tensor(pb["x_ref"]), torch.as_tensor(pb["u_ref"]), pb["Q"], pb["R"], gamma)))
            if rows is not None:
                g.append(g_of_trajectory(means, [torch.diagonal(c) for c in covs], *rows).numpy().reshape(-1))
        return np.array(cost), (np.array(g) if rows is not None else None)
    return evaluate


def solve(evaluate, U0, K, da, iterations, sigma, decay, beta, seed, call_index, lb, ub):
    """The planner's loop over ``evaluate(U (K, n)) -> (cost, g | None)``.  Returns dict(U (n,), violation, cost, trace (iterations, 6))."""
    mean = np.asarray(U0, dtype=np.float64).reshape(-1).copy()
    best = np.concatenate(([np.inf, np.inf], mean))
    trace = []
    for it in range(iterations):
        U = sample(mean, K, da, sigma, lb, ub, seed, call_index, it, decay)
        cost, g = evaluate(U)
        r = update(U, cost, g, mean, best, beta)
        mean, best = r["mean"], r["best"]
        trace.append(r["trace"])
    return {"U": best[2:].copy(), "violation": best[0], "cost": best[1], "trace": np.array(trace), "mean": mean}
