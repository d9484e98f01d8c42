"""Holds tests/gpstate_reference.py itself (CPU): the block-inverse formulas against 50-digit inverses with a NON-symmetric K, predict
and ml_grad against the float64 torch oracle, and the two conditions that make the GPU tolerances of tests/test_gpu_gpstate.py mean
something: an honest float64 evaluation sits ten-fold under them, and the inputs move by percents when a row form is exchanged for a
column form."""
import functools

import numpy as np
import pytest

import gpstate_reference as R

LD = R.DEFAULT
CAP = 1e-13              # float64 against extended precision, of the largest element: the GPU tolerance is 1e-12
SWAP_MIN = 1e-4          # what exchanging v / w, b / c or K / K^T must at least move, n >= 75


@functools.lru_cache(maxsize=None)
def _problem(n, D):
    return R.problem(R.seed_of(n, D), n, D)


def _writable(pr):
    """Copies for torch, which refuses read-only arrays."""
    return {k: np.array(v) if isinstance(v, np.ndarray) else v for k, v in pr.items()}


def _rel(a, ref):
    ref = np.asarray(ref)
    return float(np.abs(np.asarray(a, dtype=ref.dtype) - ref).max() / np.abs(ref).max())


def _mp_inverse(mp, M):
    n = len(M)
    return np.array(mp.inverse(mp.matrix(M.tolist())).tolist(), dtype=object).reshape(n, n)


def test_block_inverse_formulas_against_50_digit_inverses():
    """append / remove / replace ARE the inverses they claim, for a non-symmetric K, to 1e-25 relative."""
    import mpmath as mp
    with mp.workdps(50):
        n, D, p = 6, 2, 2
        pr = R.problem(7, n + 1, D, asym=3e-2)                         # asymmetry well above any tolerance here
        K = R.cast(np.linalg.inv(pr["Kinv"]), R.MP)[:n, :n]            # any well-conditioned non-symmetric matrix will do
        assert float(max(abs(K[i, j] - K[j, i]) for i in range(n) for j in range(n))) > 1e-2
        Kinv = _mp_inverse(mp, K)
        k = R.cast(pr["Kf"][:n, n], R.MP)
        kappa = R.cast(pr["Ky"][n, n], R.MP)

        def rel(a, b):
            return max(abs(x - y) for x, y in zip(a.ravel(), b.ravel())) / max(abs(y) for y in b.ravel())

        bordered = np.empty((n + 1, n + 1), dtype=object)
        bordered[:n, :n], bordered[:n, n], bordered[n, :n], bordered[n, n] = K, k, k, kappa
        e_app = rel(R.append(Kinv, k, kappa, R.MP), _mp_inverse(mp, bordered))
        keep = [i for i in range(n) if i != p]
        e_rem = rel(R.remove(Kinv, p, R.MP), _mp_inverse(mp, K[keep][:, keep]))
        kt = R.cast(pr["Kf"][:n, n], R.MP).copy()
        kt[p] = mp.mpf(123)                                            # entry p of kt is ignored
        Kr = K.copy()
        Kr[:, p], Kr[p, :] = k, k
        Kr[p, p] = kappa
        e_rep = rel(R.replace(Kinv, kt, kappa, p, R.MP), _mp_inverse(mp, Kr))
        # the same for the last and the first slot, and for n = 1 (nothing left of the old matrix)
        for q in (0, n - 1):
            Kq = K.copy()
            Kq[:, q], Kq[q, :] = k, k
            Kq[q, q] = kappa
            e_rep = max(e_rep, rel(R.replace(Kinv, k, kappa, q, R.MP), _mp_inverse(mp, Kq)))
            kq = [i for i in range(n) if i != q]
            e_rem = max(e_rem, rel(R.remove(Kinv, q, R.MP), _mp_inverse(mp, K[kq][:, kq])))
        one = R.replace(Kinv[:1, :1], k[:1], kappa, 0, R.MP)
        assert one.shape == (1, 1) and abs(one[0, 0] * kappa - 1) < mp.mpf(10) ** -45
        print("  50 digits, non-symmetric K: append %.1e, remove %.1e, replace %.1e" % (float(e_app), float(e_rem), float(e_rep)))
        assert e_app < mp.mpf(10) ** -25 and e_rem < mp.mpf(10) ** -25 and e_rep < mp.mpf(10) ** -25
        # and the transposed forms are NOT: v <-> w in the append, b <-> c in the removal
        assert rel(R.append(Kinv.T, k, kappa, R.MP), _mp_inverse(mp, bordered)) > 1e-3
        assert rel(R.remove(Kinv.T, p, R.MP), _mp_inverse(mp, K[keep][:, keep])) > 1e-3


def test_longdouble_and_mpmath_forms_agree():
    """The two precisions the module can run in evaluate the same lines (kernel / predict / ml_grad included)."""
    import mpmath as mp
    pr = _problem(9, 5)
    with mp.workdps(40):
        for name, args in (("append", (pr["Kinv"], pr["Kf"][0], 1.7)), ("remove", (pr["Kinv"], 4)), ("replace", (pr["Kinv"], pr["Kf"][1], 1.7, 8))):
            a, b = getattr(R, name)(*args, R.MP), getattr(R, name)(*args, LD)
            assert _rel(R.to_f64(a), R.to_f64(b)) < 1e-15, name
        a = R.predict(pr["X"], pr["lam"], pr["sf"], pr["beta"], pr["Kinv"], pr["noise"], pr["Xp"][:3], R.MP)
        b = R.predict(pr["X"], pr["lam"], pr["sf"], pr["beta"], pr["Kinv"], pr["noise"], pr["Xp"][:3], LD)
        for key in a:
            np.testing.assert_allclose(R.to_f64(a[key]), R.to_f64(b[key]), rtol=1e-14, err_msg=key)
        a = R.ml_grad(pr["X"], pr["Kinv"], pr["beta"], pr["y"], pr["lam"], pr["sf"], pr["noise"], R.MP)
        b = R.ml_grad(pr["X"], pr["Kinv"], pr["beta"], pr["y"], pr["lam"], pr["sf"], pr["noise"], LD)
        np.testing.assert_allclose(R.to_f64(a[1]), R.to_f64(b[1]), rtol=1e-14)
        assert np.abs(R.to_f64(a[0]) - R.to_f64(b[0])).max() <= 1e-15 * R.to_f64(b[1]).max()


def test_precision_of_the_reference():
    assert R.HAVE_LD == (np.finfo(np.longdouble).nmant >= 63)
    if R.HAVE_LD:
        assert R.DEFAULT is np.longdouble and np.finfo(np.longdouble).eps < 1.1e-19
    k = R.kernel(np.zeros((1, 2)), np.ones((1, 2)), [1.0, 2.0], 1.2)
    assert abs(float(k[0, 0]) - 1.44 * np.exp(-0.75)) < 1e-15 and (k.dtype == object or k.dtype == np.longdouble)


def test_ladder_has_every_dimension_and_the_schur_ladder_its_condition():
    lad, sch = R.ladder(), R.ladder(schur=True)
    assert [n for n, _ in lad] == list(R.LADDER_N) == [n for n, _ in sch]
    assert {D for _, D in lad} == set(range(1, 9))
    assert all(D >= 3 for n, D in sch if n >= 255)
    assert R.slots(1) == [0] and R.slots(2) == [0, 1] and R.slots(257) == [0, 128, 255, 256] and R.slots(256) == [0, 128, 255]


def test_predict_against_the_float64_oracle():
    """Symmetric inputs (the oracle knows nothing of asymmetry): rtol 1e-9."""
    from oracle import gpmpc_oracle as O
    for n, D, p in ((40, 3, 7), (65, 1, 9), (17, 8, 1)):
        pr = _writable(R.problem(5 + n, n, D, asym=0.0))
        sn = np.sqrt(pr["noise"])
        Xp = pr["Xp"][:p]
        mean, cov = O.predict(Xp, pr["X"], pr["y"], pr["Kinv"], pr["lam"], pr["sf"], sn, covar=True, targets=True)
        got = R.predict(pr["X"], pr["lam"], pr["sf"], pr["beta"], pr["Kinv"], pr["noise"], Xp)
        np.testing.assert_allclose(R.to_f64(got["Ks"]), O.cross_kernel(Xp, pr["X"], pr["lam"], pr["sf"]).numpy(), rtol=1e-9)
        np.testing.assert_allclose(R.to_f64(got["mean"]), mean.reshape(-1), rtol=1e-9)
        np.testing.assert_allclose(R.to_f64(got["cov"]), cov, rtol=1e-9)
        # the sums of absolute terms bound the values they accompany
        assert (np.abs(got["mean"]) <= got["mean_abs"]).all() and (np.abs(got["W"]) <= got["W_abs"]).all()
        assert (np.abs(got["cov"]) <= got["cov_abs"] + pr["noise"]).all()


def _float64_autograd_ml_grad(X, y, lam, sf, noise):
    """d ml / d log-hypers by autograd through inv / det, every factor float64 (the oracle's own noise term is a float32 product)."""
    import torch
    from oracle import gpmpc_oracle as O
    ll = torch.tensor(np.log(lam), dtype=torch.float64, requires_grad=True)
    lf = torch.tensor(np.log(sf), dtype=torch.float64, requires_grad=True)
    ln = torch.tensor(0.5 * np.log(noise), dtype=torch.float64, requires_grad=True)
    Xt, yt = torch.as_tensor(X), torch.as_tensor(y).reshape(-1, 1)
    Kf = torch.exp(lf) ** 2 * torch.exp(-0.5 * O.scaled_sqdist(Xt, Xt, torch.exp(ll)))
    Ky = Kf + torch.exp(ln) ** 2 * torch.eye(len(X), dtype=torch.float64)
    ml = -0.5 * yt.mT @ torch.linalg.inv(Ky) @ yt - 0.5 * torch.log(torch.linalg.det(Ky))
    ml.backward()
    return ll.grad.numpy(), lf.grad.item(), ln.grad.item()


def test_ml_grad_against_the_oracle_hyper_trainer():
    """ml_grad against HyperTrainer.step() (autograd through inv / det) at rtol 1e-9, symmetric inputs.  The oracle follows the
    reference in forming the noise term as a float32 product, so its Ky carries float32(sigma_n^2) -- which is what the restatement is
    given here -- and its d / d log sigma_n passes through a float32 backward (6e-8 per element): that one entry is held to step() at
    the tolerance tests/test_gpu_api.py states for this path (2e-6), and at 1e-9 to the same autograd with a float64 noise term."""
    from oracle import gpmpc_oracle as O
    for n, D in ((37, 2), (64, 1), (130, 5), (9, 8)):
        pr = _writable(R.problem(11 + n, n, D, asym=0.0))
        ln = 0.5 * np.log(pr["noise"])
        tr = O.HyperTrainer(pr["X"], pr["y"], D, log_lambdas=np.log(pr["lam"]), log_sigma_f=np.log(pr["sf"]), log_sigma_n=ln)
        lam, sf = np.exp(np.log(pr["lam"])), float(np.exp(np.log(pr["sf"])))
        _, Ky, Kinv = O.kernel_matrices(pr["X"], lam, sf, float(np.exp(ln)))
        noise32 = float(Ky[0, 0]) - sf ** 2
        assert abs(noise32 / pr["noise"] - 1) < 1e-7
        Kinv = Kinv.numpy()
        ref = tr.step()["grad"]
        alpha = Kinv @ pr["y"]
        val, mag = R.ml_grad(pr["X"], Kinv, alpha, pr["y"], lam, sf, noise32)
        val = R.to_f64(val)
        assert (np.abs(val) <= R.to_f64(mag)).all()
        print("  n %3d D %d: lambda %.1e, sigma_f %.1e, sigma_n %.1e against step()" % (
            n, D, np.abs(val[:D] / ref["log_lambdas"] - 1).max(), abs(val[D] / ref["log_sigma_f"] - 1), abs(val[D + 1] / ref["log_sigma_n"] - 1)))
        np.testing.assert_allclose(val[:D], ref["log_lambdas"], rtol=1e-9)
        np.testing.assert_allclose(val[D], ref["log_sigma_f"], rtol=1e-9)
        np.testing.assert_allclose(val[D + 1], ref["log_sigma_n"], rtol=2e-6)
        np.testing.assert_allclose(val[D + 2], pr["y"] @ alpha, rtol=1e-12)
        g_lam, g_f, g_n = _float64_autograd_ml_grad(pr["X"], pr["y"], lam, sf, noise32)
        np.testing.assert_allclose(val[:D], g_lam, rtol=1e-9)
        np.testing.assert_allclose([val[D], val[D + 1]], [g_f, g_n], rtol=1e-9)


def _append_vw_swapped(Kinv, k, kappa, prec):
    """The append with v and w exchanged (what exchanging acc[0] and acc[1] in k_append_vw2 computes)."""
    Kinv, k = R.cast(Kinv, prec), R.cast(k, prec)
    n = len(k)
    w, v = Kinv @ k, Kinv.T @ k                                        # exchanged
    q = 1 / (kappa - k @ v)
    out = np.empty((n + 1, n + 1), dtype=Kinv.dtype)
    out[:n, :n], out[:n, n], out[n, :n], out[n, n] = Kinv + q * np.outer(v, w), -q * v, -q * w, q
    return out


def _remove_bc_swapped(Kinv, p, prec):
    """The removal with b = K[p, :] and c = K[:, p] (what reading p * ld_in + i for ld_in * i + p in k_kinv_remove computes)."""
    Kinv = R.cast(Kinv, prec)
    A = Kinv - np.outer(Kinv[p, :], Kinv[:, p]) / Kinv[p, p]
    keep = [i for i in range(len(Kinv)) if i != p]
    return A[keep][:, keep]


@pytest.mark.parametrize("n,D", R.ladder(schur=True))
def test_float64_sits_tenfold_under_the_gpu_tolerance_and_the_inputs_see_a_swap(n, D):
    """For every Schur-update case of the GPU ladder: a plain float64 numpy evaluation of the same formulas differs from the extended
    one by at most 1e-13 of the largest element (the GPU tolerance is 1e-12: an honest float64 implementation has ten-fold room,
    nothing looser passes), and for n >= 75 exchanging v / w, b / c or feeding K^T moves the result by more than 1e-4."""
    pr = _problem(n, D)
    Kinv, kappa = pr["Kinv"], pr["sf"] ** 2 + pr["noise"]
    k = R.to_f64(R.kernel(pr["X"], pr["xnew"][None, :], pr["lam"], pr["sf"]))[:, 0]
    ref = R.append(Kinv, k, kappa)
    err = {"append": _rel(R.append(Kinv, k, kappa, np.float64), ref)}
    swap = {"append": _rel(_append_vw_swapped(Kinv, k, kappa, np.float64), ref), "append K^T": _rel(R.append(Kinv.T, k, kappa, np.float64), ref)}
    err["remove"], err["replace"], swap["remove"], swap["replace K^T"] = 0.0, 0.0, np.inf, np.inf
    for p in R.slots(n):
        kt = k.copy()
        kt[p] = 0.0
        ref = R.replace(Kinv, kt, kappa, p)
        err["replace"] = max(err["replace"], _rel(R.replace(Kinv, kt, kappa, p, np.float64), ref))
        swap["replace K^T"] = min(swap["replace K^T"], _rel(R.replace(Kinv.T, kt, kappa, p, np.float64), ref))
        if n >= 2:
            ref = R.remove(Kinv, p)
            err["remove"] = max(err["remove"], _rel(R.remove(Kinv, p, np.float64), ref))
            swap["remove"] = min(swap["remove"], _rel(_remove_bc_swapped(Kinv, p, np.float64), ref))
    print("  n %3d D %d  float64 vs extended: append %.1e remove %.1e replace %.1e | swap moves: append %.1e (K^T %.1e) remove %.1e replace K^T %.1e"
          % (n, D, err["append"], err["remove"], err["replace"], swap["append"], swap["append K^T"], swap["remove"], swap["replace K^T"]))
    for name, e in err.items():
        assert e <= CAP, (name, e)
    if n >= 75:
        for name, s in swap.items():
            assert s > SWAP_MIN, (name, s)
