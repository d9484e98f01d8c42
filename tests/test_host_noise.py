"""CPU-only tests of the noise model of the rollout (init_cov, action_var, process_var): the float64 reference of the GPU tests
(tests/noise_reference.py) against the pinned oracle -- equal at the defaults, and moved by each part alone by at least ten of the GPU
tolerances on the very problems tests/test_gpu_noise.py runs --; the two C ABI entry points are exported, declared and refuse bad values
before any device call; the Python objects validate shapes."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import offgrid_problems as OG
import noise_reference as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpmpc_pack_set_noise", "gpmpc_pack_get_noise")
DIMS = [(1, 1), (2, 2), (4, 1), (7, 1)]
MEAN_RTOL, VAR_RTOL, COST_RTOL, GRAD_RTOL = OG.GPU_MEAN_RTOL, OG.GPU_VAR_RTOL, OG.GPU_COST_RTOL, OG.GPU_GRAD_RTOL
_refs = {}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import gaussian_process_mpc_amd as g
    return g


def _problem(ds, da):
    from oracle import gpmpc_oracle as O
    args = (OG.ladder_config(ds, da), OG.LADDER_N, ds, da, OG.LADDER_H, OG.ladder_batches(ds)["big"], False)
    pb, kinv = OG.problem(*args)
    return pb, O.GPBundle(pb["X"], pb["Y"], pb["lambdas"], pb["sigma_f"], pb["sigma_n"], Ky_inv=kinv)


def _ref(ds, da, which, fullcov=False, b=0):
    """Trajectory b of a ladder problem under one model: "default", "all", or one part of ``ladder_noise`` alone; once per module."""
    key = (ds, da, which, fullcov, b)
    if key not in _refs:
        pb, gp = _problem(ds, da)
        P, av, w = NR.ladder_noise(ds, da)
        kw = {"default": {}, "all": dict(init_cov=P, action_var=av, process_var=w), "init_cov": dict(init_cov=P),
              "action_var": dict(action_var=av), "process_var": dict(process_var=w)}[which]
        _refs[key] = NR.rollout(gp, pb["H"], pb["x0"][b], pb["U"][b], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], -1.0, fullcov=fullcov, **kw)
    return _refs[key]


def _excess(a, b, rtol, atol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (atol + rtol * np.abs(b))))


def _moved(r, d, fullcov=False):
    """How far result r is from d, per output, in units of the GPU tests' tolerance for that output."""
    out = {"means": _excess(r["means"], d["means"], MEAN_RTOL, 1e-9), "cost": _excess(r["cost"], d["cost"], COST_RTOL, 0.0),
           "grad": float(np.linalg.norm(r["grad"] - d["grad"]) / np.linalg.norm(d["grad"]) / GRAD_RTOL)}
    if fullcov:
        out["covs"] = _excess(r["covs"], d["covs"], VAR_RTOL, 1e-6 * np.abs(d["covs"]).max())
    else:
        out["vars"] = _excess(r["vars"], d["vars"], VAR_RTOL, 1e-12)
    return out


@pytest.mark.parametrize("ds,da", DIMS)
def test_reference_equals_the_oracle_at_the_defaults(ds, da):
    """With nothing set -- and with the defaults passed explicitly -- the restated loops ARE the oracle's: every output equal, not close."""
    from oracle import gpmpc_oracle as O
    pb, gp = _problem(ds, da)
    H = pb["H"]
    o = O.objective_and_gradient(gp, H, pb["x0"][0], pb["U"][0], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], -1.0, mode="o2")
    f = O.objective_and_gradient_fullcov(gp, H, pb["x0"][0], pb["U"][0], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], -1.0)
    P, av, w = NR.defaults(ds, da)
    for kw in ({}, dict(init_cov=P, action_var=av, process_var=w), dict(init_cov=np.diag(P))):
        r = NR.rollout(gp, H, pb["x0"][0], pb["U"][0], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], -1.0, **kw)
        g = NR.rollout(gp, H, pb["x0"][0], pb["U"][0], pb["x_ref"], pb["u_ref"], pb["Q"], pb["R"], -1.0, fullcov=True, **kw)
        for k in ("means", "vars", "grad"):
            assert np.array_equal(r[k], o[k]), (k, np.abs(r[k] - o[k]).max())
        for k in ("means", "covs", "grad"):
            assert np.array_equal(g[k], f[k]), (k, np.abs(g[k] - f[k]).max())
        assert r["cost"] == o["cost"] and g["cost"] == f["cost"]


@pytest.mark.parametrize("ds,da", DIMS)
def test_each_part_alone_moves_the_reference_by_ten_tolerances(ds, da):
    """What makes tests/test_gpu_noise.py discriminating: on ITS problems and ITS model, init_cov alone, action_var alone and process_var alone
    each move some output of the diagonal AND of the full-covariance reference by >= 10 of that output's GPU tolerance -- a kernel that
    ignores a part misses by that factor.  All three together: asserted too; and from ds = 2 the off-diagonal init_cov and the
    cross-covariances move the full-covariance diagonal away from the diagonal rollout by >= 10 tolerances (at ds = 1 they coincide)."""
    for fullcov in (False, True):
        d = _ref(ds, da, "default", fullcov)
        for which in ("init_cov", "action_var", "process_var", "all"):
            r = _ref(ds, da, which, fullcov)
            if fullcov:
                OG.assert_fullcov_reference_is_sane(r["means"], r["covs"], r["cost"])
            else:
                OG.assert_diag_reference_is_sane(r["means"], r["vars"], r["cost"], _problem(ds, da)[0]["Q"], -1.0)
            mv = _moved(r, d, fullcov)
            print("ds=%d da=%d %s %s moves (in tolerances):" % (ds, da, "fullcov" if fullcov else "diag", which), {k: "%.3g" % v for k, v in mv.items()})
            assert max(mv.values()) >= 10.0, (which, fullcov, mv)
    a, f = _ref(ds, da, "all", False), _ref(ds, da, "all", True)
    fd = np.stack([np.diag(c) for c in f["covs"]])
    gap = _excess(fd[1:], a["vars"][1:], VAR_RTOL, 1e-12)
    print("ds=%d: full-covariance diagonal against the diagonal rollout: %.3g tolerances" % (ds, gap))
    if ds == 1:
        assert np.array_equal(fd, a["vars"])
    else:
        assert gap >= 10.0, gap


@pytest.mark.parametrize("ds,da", DIMS)
def test_process_var_enters_step_one_additively(ds, da):
    """Step 1 sees the same input distribution with and without process_var: var_1(w) - var_1(0) = w up to the rounding of one addition, the
    means of step 1 are unchanged; from step 2 on both move."""
    w = NR.ladder_noise(ds, da)[2]
    for fullcov in (False, True):
        d, r = _ref(ds, da, "default", fullcov), _ref(ds, da, "process_var", fullcov)
        v0 = d["vars"][1] if not fullcov else np.diag(d["covs"][1])
        v1 = r["vars"][1] if not fullcov else np.diag(r["covs"][1])
        np.testing.assert_allclose(v1 - v0, w, rtol=0, atol=4 * np.finfo(np.float64).eps * np.abs(v1).max())
        assert np.array_equal(r["means"][:2], d["means"][:2])
        assert not np.array_equal(r["means"][2], d["means"][2])
        if fullcov and ds > 1:                               # an additive DIAGONAL term: the cross-covariances of step 1 stay
            off = ~np.eye(ds, dtype=bool)
            assert np.array_equal(r["covs"][1][off], d["covs"][1][off])


def test_noise_symbols_are_exported_and_declared(built):
    from gaussian_process_mpc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gpmpc_[a-z_]+)\s*\(", hdr))
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(h, name) is not None
        assert getattr(built.lib(), name).argtypes == _lib.SIGNATURES[name][1]


def _fake_pack(ds, da):
    """Host memory that stands in for a pack where only its dimensions are read (the leading ints of the struct: N, Np, ds, da, D), zero
    elsewhere: every call below is refused before the first device call, and a call that were not refused finds a null device buffer."""
    buf = ctypes.create_string_buffer(1 << 20)
    ctypes.memmove(buf, (ctypes.c_int * 5)(64, 64, ds, da, ds + da), 5 * ctypes.sizeof(ctypes.c_int))
    return buf


def test_noise_argument_validation_without_device(built):
    lib = built.lib()
    dbl = lambda a: (ctypes.c_double * len(a))(*[float(v) for v in a])  # noqa: E731
    assert lib.gpmpc_pack_set_noise(None, None, None, None, None) == -1      # GPMPC_E_ARG: no pack
    assert lib.gpmpc_pack_get_noise(None, None, None, None) == -1
    ds, da = 3, 2
    pack = _fake_pack(ds, da)
    P = np.array([[2e-2, 1e-3, 0.0], [1e-3, 1e-2, -2e-3], [0.0, -2e-3, 3e-2]])
    av, w = [1e-3, 0.0], [1e-4, 0.0, 2e-3]
    setn = lambda P_=P, av_=av, w_=w: lib.gpmpc_pack_set_noise(pack, None if P_ is None else dbl(np.asarray(P_).reshape(-1)),  # noqa: E731
                                                               None if av_ is None else dbl(av_), None if w_ is None else dbl(w_), None)
    err = lambda: lib.gpmpc_last_error().decode()  # noqa: E731
    for bad in (float("nan"), float("inf"), -float("inf")):
        Q = P.copy()
        Q[1, 1] = bad
        assert setn(P_=Q) == -1 and "init_cov" in err() and "finite" in err(), err()
        Q = P.copy()
        Q[0, 2] = Q[2, 0] = bad
        assert setn(P_=Q) == -1 and "finite" in err()
        assert setn(av_=[1e-3, bad]) == -1 and "action_var[1]" in err(), err()
        assert setn(w_=[bad, 0.0, 0.0]) == -1 and "process_var[0]" in err(), err()
    Q = P.copy()
    Q[2, 2] = -1e-9
    assert setn(P_=Q) == -1 and "init_cov[2][2]" in err() and "negative" in err(), err()
    assert setn(av_=[-1e-12, 0.0]) == -1 and "action_var[0]" in err() and "negative" in err(), err()
    assert setn(w_=[0.0, 0.0, -1e-300]) == -1 and "process_var[2]" in err() and "negative" in err(), err()
    Q = P.copy()
    Q[0, 1] += 2e-12 * np.abs(P).max()                      # beyond 1e-12 max |P|
    assert setn(P_=Q) == -1 and "symmetric" in err(), err()
    # each part is checked whether or not the others are given
    assert setn(P_=None, av_=None, w_=[0.0, float("nan"), 0.0]) == -1 and setn(P_=None, av_=[0.0, -1.0], w_=None) == -1
    Q = P.copy()
    Q[0, 0] = -1.0
    assert setn(P_=Q, av_=None, w_=None) == -1


def test_python_objects_validate_shapes(built):
    from gaussian_process_mpc_amd.rollout import noise_arrays
    P, av, w = noise_arrays(3, 2, [1e-2, 2e-2, 3e-2], 1e-3, [0.0, 1e-4, 0.0])
    np.testing.assert_array_equal(P, np.diag([1e-2, 2e-2, 3e-2]))            # a vector is a diagonal
    np.testing.assert_array_equal(av, [1e-3, 1e-3])
    np.testing.assert_array_equal(w, [0.0, 1e-4, 0.0])
    assert P.flags["C_CONTIGUOUS"] and P.dtype == np.float64
    assert noise_arrays(3, 2) == (None, None, None)
    M = np.arange(9.0).reshape(3, 3)
    np.testing.assert_array_equal(noise_arrays(3, 2, init_cov=M)[0], M)      # (values are the library's business)
    np.testing.assert_array_equal(noise_arrays(2, 1, init_cov=0.5)[0], 0.5 * np.eye(2))
    for kw in (dict(init_cov=np.zeros(2)), dict(init_cov=np.zeros((3, 2))), dict(init_cov=np.zeros((2, 2))), dict(init_cov=np.zeros((1, 3, 3))),
               dict(action_var=np.zeros(3)), dict(action_var=np.zeros((2, 1))), dict(process_var=np.zeros(2)), dict(process_var=np.zeros((3, 1)))):
        with pytest.raises(ValueError):
            noise_arrays(3, 2, **kw)
    # "sigma_n" is understood where the GPs are known, not by a pack
    pack = object.__new__(built.GPPack)
    pack.ds, pack.da, pack._h = 2, 1, None
    with pytest.raises(ValueError, match="sigma_n"):
        pack.set_noise(process_var="sigma_n")
    d = object.__new__(built.Dynamics)
    d.state_dim, d.action_dim, d._pack, d.gpr_err = 2, 1, None, []
    d.set_noise_model(init_cov=[1e-2, 2e-2], process_var="sigma_n")
    np.testing.assert_array_equal(d._noise[0], np.diag([1e-2, 2e-2]))
    assert d._noise[1] is None and d._noise[2] == "sigma_n" and d._noise_applied is None
    with pytest.raises(ValueError):
        d.set_noise_model(process_var="sigma_f")
    with pytest.raises(ValueError):
        d.set_noise_model(init_cov=np.zeros(3))
    with pytest.raises(ValueError, match="finite"):
        d.set_noise_model(action_var=[float("nan")])
    assert d._noise[2] == "sigma_n"                                          # a refused call leaves the stored model
    d.set_noise_model()
    assert d._noise == (None, None, None)
    assert isinstance(built.GPPack.noise, property)
    for cls, names in ((built.GPPack, ("set_noise",)), (built.Dynamics, ("set_noise_model",)),
                       (built.RiskSensitiveMPC, ("set_noise_model", "set_initial_covariance"))):
        for n in names:
            sig = inspect.signature(getattr(cls, n))
            assert all(p.default is None for k, p in sig.parameters.items() if k in ("init_cov", "action_var", "process_var")), (cls, n)
