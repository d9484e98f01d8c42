"""The WIDE cases of the model-based rollouts (csrc/linprop.hip, linprop_stream.hip, linprop_fc.hip, linprop_inputs.hip and the particle
kernels): D = state_dim + action_dim of 6, 7 and 8, state_dim from 2 to 8, action_dim from 0 to 5.  The inputs of
tests/test_host_linprop_wide.py (which pins the references, the controls and the conditioning of the chains on them, on the CPU) and of
tests/test_gpu_linprop_wide.py (which holds the kernels to the references on them).  A plain helper module in the manner of
tests/offgrid_problems.py: no fixtures, no collection hooks.  Everything is built on ``linprop_reference.make_model``; every draw is a
function of the case's name alone, so both files see the same numbers.

Each case is the smallest one for what its ``why`` names.  ``n`` crosses a 64-row block with a ragged 16-deep stage (70), three row
blocks (130) or sits on the block edge (64); B = 3 is one padded column tile, B = 5 is GPMPC_LINPROP_STREAM_COLS + 1, B = 65 two tiles."""
import functools

import numpy as np

import linprop_fc_reference as F
import linprop_reference as R

WIDE = {
    "w1": dict(n=70, ds=5, da=3, B=3, H=3,
               why="D = 8 instance of k_lpf_hess (its largest LDS); DS = 5 sweeps; STREAM groups per GP; a ragged 16-deep stage"),
    "w2": dict(n=130, ds=7, da=1, kind="shared", B=5, H=2,
               why="p = 35, nc = 36; DS = 7 sweeps; ONE inverse: 35 STREAM vectors in 9 groups of 4 that straddle columns, the last of 3; "
                   "three row blocks"),
    "w3": dict(n=70, ds=6, da=2, groups=((0, 2, 5), (1, 4), (3,)), nominal=True, noise=True, B=3, H=3, schedule=True,
               why="three GpGroups with gaps, one of three members; DS = 6; nominal weights at D = 8; a non-diagonal init_cov"),
    "w4": dict(n=64, ds=8, da=0, B=3, H=2,
               why="action_dim = 0: U is NULL, p = 44, a 44 x 44 packed Jacobian, no gain, no cost"),
    "w5": dict(n=70, ds=4, da=4, B=65, H=2,
               why="two column tiles, and chunk = 64 with a one-column second chunk, at D = 8; DS = 4"),
    "w6": dict(n=70, ds=2, da=5, B=3, H=13,
               why="D = 7 instance; H da = 65: two waves in both constraint sweeps, tau = c / 5 crossing the wave edge"),
    "w7": dict(n=70, ds=3, da=3, kind="nonsym", B=3, H=3,
               why="D = 6 instance; r = (K + K^T) k at three inputs"),
}
NAMES = list(WIDE)
FORMS = ["tile", "stream"]
# the deliberate mistakes of the references (their docstrings) and the cases each is held against
STEP_CONTROLS = {"w1": "drop_h", "w5": "drop_h", "w3": "drop_nominal_g", "w7": "r_twice"}
FULL_CONTROLS = {"w1": "drop_cross_hess", "w2": "offdiag_once", "w3": "feedback_cross_dropped", "w6": "feedback_cross_dropped"}
INPUT_CONTROLS = {"w1": "R_transposed", "w6": "gain_of_next_step"}
PER_STEP_GAIN = ("w1", "w3", "w6")                       # a gain (H, da, ds) in the rollouts; the others take one (da, ds)
INPUT_CASES = ("w1", "w3", "w6")                         # the commanded input: input cost and input chance constraints
PARTICLE_DIMS = [(3, 3), (5, 3)]                         # the particle step; (5, 3) also the inputs under feedback
PARTICLE_N = PARTICLE_P = 70
# The generator seeds of ``problem``.  The rollouts: 11, the seed of the neighbouring GPU files.  The commanded input: theirs is 23, at which
# one input radicand of w6 (13 steps of per-step gains at ds = 2) falls to 8.7e-4, below the 1e-3 tests/test_host_linprop_wide.py keeps
# every propagated radicand above; 24 is the next seed at which all three cases hold it (smallest 6.3e-3).  Chosen on the CPU reference.
ROLLOUT_SEED, INPUT_SEED = 11, 24
K95 = 1.6448536269514722                                 # the 95 % quantile of the standard normal


def dims_of(name):
    c = WIDE[name]
    return c["ds"], c["da"], c["B"], c["H"]


@functools.lru_cache(maxsize=None)
def model(name):
    """The case's model (shared: do not write to it)."""
    c = WIDE[name]
    return R.make_model(c["n"], c["ds"], c["da"], kind=c.get("kind", "pergp"), noise=c.get("noise", False), nominal=c.get("nominal", False),
                        groups=c.get("groups"))


@functools.lru_cache(maxsize=None)
def roll_model(name):
    """The model of the rollouts: w3 starts from a non-diagonal SPD init_cov (the recipe of tests/test_gpu_linprop_fc.py's roll_model)."""
    m = dict(model(name))
    if name == "w3":
        ds = WIDE[name]["ds"]
        A = np.random.default_rng(4).standard_normal((ds, ds))
        P0 = 2e-3 * (A @ A.T) / ds + 1e-3 * np.eye(ds)
        m["init_cov"] = 0.5 * (P0 + P0.T)
    return m


class _HostCost:
    """Stands where the package does in ``cost_case`` when no device is there: the draws are made, nothing is built."""

    class CostSchedule:
        def __init__(self, *a):
            pass

        def set(self, *a):
            return self

    @staticmethod
    def CostParams(*a, **kw):
        return None


def cost_draws(name, rng):
    """(gamma, Q, R), the keyword arguments of cost_reference: the draws of tests/test_gpu_linprop.py's ``cost_case`` from ``rng``."""
    import test_gpu_linprop as TL
    _, gqr, kw = TL.cost_case(_HostCost, roll_model(name), WIDE[name]["H"], rng, WIDE[name].get("schedule", False))
    return gqr, kw


def state_rows(ds):
    """Three rows: an axis row at 95 %, a general row at kappa = 2, a mean-only row (``_rows`` of tests/test_gpu_mppi.py)."""
    rng = np.random.default_rng(77 + ds)
    A = rng.standard_normal((3, ds))
    A[0] = 0.0
    A[0, 0] = 1.0
    return A, np.array([0.5, 0.2, 0.1]), np.array([K95, 2.0, 0.0])


def input_rows(da, rng):
    """Two rows on the commanded input: an upper bound on the first input, one that is not axis-aligned."""
    C = np.concatenate([np.eye(da)[:1], rng.uniform(0.3, 1.0, (1, da)) * np.where(np.arange(da) % 2, -1.0, 1.0)])
    return C, np.array([1.5, 0.8]), np.array([1.6, 2.0])


def plans(name, seed=ROLLOUT_SEED):
    """x0 (B, ds), U (B, H, da) and the gain: (H, da, ds) on PER_STEP_GAIN, (da, ds) elsewhere, None at da = 0.  The long horizon of w6
    (H = 13) keeps its plans small, so that the chain stays in the data's range (tests/test_gpu_feedback_inputs.py does the same)."""
    ds, da, B, H = dims_of(name)
    rng = np.random.default_rng(seed)
    x0, U = rng.uniform(-1.0, 1.0, (B, ds)), rng.uniform(-1.0, 1.0, (B, H, da))
    if H > 3:
        U = 0.3 * U
    K = None if da == 0 else rng.uniform(-0.5, 0.5, (H, da, ds) if name in PER_STEP_GAIN else (da, ds))
    return x0, U, K


def problem(name, seed=ROLLOUT_SEED):
    """Everything a rollout test draws: ``plans`` (x0, U, K), the three state rows, and at action_dim >= 1 the cost (the draws of
    ``cost_case`` from the generator seeded ``cost_seed``) and the two input rows: dict(x0, U, K, rows) + dict(gamma, Q, R, cost_kw, C, d,
    kappa_u, cost_seed).  seed: ROLLOUT_SEED or INPUT_SEED."""
    x0, U, K = plans(name, seed)
    pb = dict(x0=x0, U=U, K=K, rows=state_rows(WIDE[name]["ds"]))
    if WIDE[name]["da"]:
        (gamma, Q, Rm), kw = cost_draws(name, np.random.default_rng(seed + 1000))
        C, d, kappa = input_rows(WIDE[name]["da"], np.random.default_rng(seed + 2000))
        pb.update(gamma=gamma, Q=Q, R=Rm, cost_kw=kw, C=C, d=d, kappa_u=kappa, cost_seed=seed + 1000)
    return pb


def embed_diag(vars_, jac, ds, da):
    """The diagonal rule in the packed layout of linprop_fc_reference: covs = diag(vars) and the step Jacobians [2ds][2ds+da] placed on
    the rows / columns (mu, Sigma_kk, u) of [p][p+da], zeros elsewhere.  ``F.constraints`` on them IS the diagonal rule's forward sweep
    (q = sum_k a_k^2 var_k: the off-diagonal variables are zero and stay zero), with its units."""
    vars_, jac = np.asarray(vars_), np.asarray(jac)
    p = F.packed_dim(ds)
    pairs = F.tri_pairs(ds)
    idx = list(range(ds)) + [ds + pairs.index((k, k)) for k in range(ds)]
    cols = idx + [p + j for j in range(da)]
    covs = np.zeros(vars_.shape + (ds,), dtype=vars_.dtype)
    for k in range(ds):
        covs[..., k, k] = vars_[..., k]
    J = np.zeros(jac.shape[:2] + (p, p + da), dtype=jac.dtype)
    J[:, :, np.asarray(idx)[:, None], np.asarray(cols)[None, :]] = jac
    return covs, J
