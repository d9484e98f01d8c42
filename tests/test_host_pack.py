"""The conditions the budget of tests/test_gpu_pack.py rests on, checked without a GPU.

1. The yardstick is pinned: tests/pack_reference.py evaluated with mpmath (prec="mp", 50 digits) agrees to 1e-25 of the unit with a second,
   element-by-element statement of the definitions, and the long double evaluation the GPU test is judged against lies within 0.01 unit
   (2^-53 A) of it, on the three smallest cases of the ladder.
2. K_ref -- the same formulas in plain float64 against the extended evaluation, in units of 2^-53 A -- on every case of the ladder.
   Measured here (18 cases, D = 1 ... 8, ds = 1 ... 8):  beta 0.35 ... 4.8,  beta of a nominal pack 0.24 ... 3.8,  weights 0.10 ... 3.0,
   with sum|terms| / |beta| from 1 (N = 1) to 3.6e4 and exponents up to 14.4: the units hold over that range of conditioning.  Asserted:
   the generous ceilings K_REF_MAX, nothing tighter (BLAS sums in an order of its own).
3. The budget DISCRIMINATES.  Each defect below is emulated in the float64 evaluation and put before both assertions: the present one
   (tests/test_gpu_parity.py::test_pack_constants: rtol 1e-9, atol 1e-9 x max, on its own fixture g3 -- N = 100, sigma_f = 1, Ky_inv
   symmetric to 4e-12) and the new one (every ladder case the defect applies to; K against min(10 K_ref, cap) as the GPU test asserts).
       defect                                   present band (g3)      new budget (worst K over the ladder: smallest ... largest)
       beta from K^T y                          passes                 misses on every case, K 7e12 ... 3e15
       weight from K_ij alone                   passes                 misses on every case
       weight from K_ji alone                   passes                 misses on every case
       sigma_f^2 for sigma_f^4                  passes (sigma_f = 1)   misses on every case
       lambda of GP 0 for every GP              CATCHES it             misses (cases with ds >= 2 and distinct lambdas)
       weight stored at the transposed place    CATCHES it             misses (the lower triangle is not zero)
       one beta term dropped (the largest the   CATCHES it: on g3 it    misses on the one ladder case where the band passes a term at all
         1e-9 band still passes)                passes no term at all  (N = 520, K = 1.9e6); elsewhere the band passes none either
       exponent rounded to float32              CATCHES it             misses on every case with N >= 2, K 2.6e7 ... 4.3e8
   OLD_BAND_CATCHES states the middle column and is asserted to be exact; the right column is asserted case by case."""
import functools

import numpy as np
import pytest

import gpstate_reference as R
import pack_reference as P

CASES = P.ladder()
IDS = [P.case_id(c) for c in CASES]
K_REF_MAX = {"beta": 10.0, "nominal": 10.0, "M": 6.0}

DEFECTS = ("beta from K^T y", "weight from K_ij alone", "weight from K_ji alone", "sigma_f^2 for sigma_f^4", "lambda of GP 0 for every GP",
           "weight stored at the transposed place", "one beta term dropped", "exponent rounded to float32")
OLD_BAND_CATCHES = {"lambda of GP 0 for every GP", "weight stored at the transposed place", "exponent rounded to float32", "one beta term dropped"}


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the yardstick is pinned
# ------------------------------------------------------------------------------------------------------------------------------
def _mp_of_longdouble(a):
    """An array of the default precision as exact mpf values (a long double is the sum of two doubles)."""
    import mpmath as mp
    if a.dtype == object:
        return a
    hi = a.astype(np.float64)
    lo = (a - hi.astype(a.dtype)).astype(np.float64)
    return np.frompyfunc(lambda h, l: mp.mpf(float(h)) + mp.mpf(float(l)), 2, 1)(hi, lo)


@pytest.mark.parametrize("case", CASES[:3], ids=IDS[:3])
def test_reference_against_a_second_evaluation_at_50_digits(case):
    import mpmath as mp
    pr = P.problem(*case)
    n, D, ds = pr["n"], pr["D"], pr["ds"]
    X, Y, Kinv, lam, sf, W, c = (pr[k] for k in ("X", "Y", "Kinv", "lam", "sf", "W", "c"))
    b64 = R.to_f64(P.beta(Kinv, Y, np.float64)[0])
    with mp.workdps(50):
        f = lambda v: mp.mpf(float(v))  # noqa: E731
        b_mp, A_b = P.beta(Kinv, Y, R.MP)
        n_mp, A_n = P.beta_nominal(Kinv, X, Y, W, c, R.MP)
        M_mp, A_M = P.weights(X, Kinv, b64, lam, sf, R.MP)
        worst = mp.mpf(0)
        for a in range(ds):
            for i in range(n):
                # the definitions, element by element, nothing shared with the module but the inputs
                s = sum((f(Kinv[a, i, j]) * f(Y[j, a]) for j in reversed(range(n))), mp.mpf(0))
                sa = sum((abs(f(Kinv[a, i, j]) * f(Y[j, a])) for j in reversed(range(n))), mp.mpf(0))
                res = [f(Y[j, a]) - sum((f(X[j, k]) * f(W[a, k]) for k in reversed(range(D))), mp.mpf(0)) - f(c[a]) for j in range(n)]
                rho = [abs(f(Y[j, a])) + sum((abs(f(X[j, k]) * f(W[a, k])) for k in reversed(range(D))), mp.mpf(0)) + abs(f(c[a])) for j in range(n)]
                sn = sum((f(Kinv[a, i, j]) * res[j] for j in reversed(range(n))), mp.mpf(0))
                sna = sum((abs(f(Kinv[a, i, j])) * rho[j] for j in reversed(range(n))), mp.mpf(0))
                worst = max(worst, abs(b_mp[a, i] - s) / sa, abs(A_b[a, i] - sa) / sa, abs(n_mp[a, i] - sn) / sna, abs(A_n[a, i] - sna) / sna)
                for j in range(n):
                    if j < i:
                        assert M_mp[a, i, j] == 0 and A_M[a, i, j] == 0
                        continue
                    e = sum(((f(X[i, k]) - f(X[j, k])) ** 2 / f(lam[a, k]) for k in reversed(range(D))), mp.mpf(0)) / 4
                    ks = (f(Kinv[a, i, j]) + f(Kinv[a, j, i])) / 2
                    bb = f(b64[a, i]) * f(b64[a, j])
                    g = (1 if i == j else 2) * f(sf[a]) ** 4 * mp.exp(-e)
                    unit = g * (abs(ks) + abs(bb) + abs(ks - bb) * (1 + e))
                    worst = max(worst, abs(M_mp[a, i, j] - g * (ks - bb)) / unit, abs(A_M[a, i, j] - unit) / unit)
        # ... and the precision the GPU test is judged against, in the unit of the budget
        b_ld, _ = P.beta(Kinv, Y)
        n_ld, _ = P.beta_nominal(Kinv, X, Y, W, c)
        M_ld, _ = P.weights(X, Kinv, b64, lam, sf)
        up = np.triu(np.ones((n, n), dtype=bool))
        k_ld = max(float((abs(_mp_of_longdouble(b_ld) - b_mp) / (A_b * P.U53)).max()), float((abs(_mp_of_longdouble(n_ld) - n_mp) / (A_n * P.U53)).max()),
                   max(float((abs(_mp_of_longdouble(M_ld[a]) - M_mp[a])[up] / (A_M[a][up] * P.U53)).max()) for a in range(ds)))
    print("  %s: mpmath form vs element-by-element definitions %.1e of the unit; default precision vs mpmath: K = %.2g" % (P.case_id(case), float(worst), k_ld))
    assert worst < mp.mpf(10) ** -25
    assert k_ld < 0.01


def test_ladder_covers_every_edge_and_dimension():
    lad = P.ladder()
    assert [c[0] for c in lad] == list(P.LADDER_N)
    for edge in (32, 64, 128, 256):
        assert {edge - 1, edge, edge + 1} <= set(P.LADDER_N)
    assert {c[1] for c in lad} == set(range(1, 9))
    assert all(1 <= c[2] <= min(c[1], 8) for c in lad)
    assert any(c[1] == c[2] for c in lad) and any(c[2] == 8 for c in lad) and any(c[2] == 1 for c in lad)        # action_dim = 0, ds = 8, no pair
    assert sum(c[3] for c in lad) >= 3 and all(c[2] >= 2 for c in lad if c[3])
    assert max((-(-c[0] // 64) * 64) ** 2 * c[2] for c in lad) <= 576 * 576 * 8
    for c in lad:
        pr = P.problem(*c)
        asym = np.abs(pr["Kinv"] - pr["Kinv"].transpose(0, 2, 1)).max() / np.abs(pr["Kinv"]).max()
        assert c[0] == 1 or asym > 1e-5, (c, asym)                                                               # genuinely non-symmetric
        assert (pr["sf"] >= P.SIGMA_F_RANGE[0]).all() and (pr["sf"] <= P.SIGMA_F_RANGE[1]).all() and np.abs(pr["sf"] - 1).min() > 1e-3
        lam_same = all(np.array_equal(pr["lam"][a], pr["lam"][0]) for a in range(c[2]))
        assert lam_same == (c[3] or c[2] == 1)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. K_ref on every case of the ladder
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_k_ref_of_the_plain_float64_evaluation(case):
    k = P.k_ref(*case)
    print("K_REF %s: beta %.3g  nominal beta %.3g  M %.3g;  sum|terms| / |beta| up to %.3g, exponents up to %.3g"
          % (P.case_id(case), k["beta"], k["nominal"], k["M"], k["cancel"], k["emax"]))
    for q, cap in K_REF_MAX.items():
        assert 0 <= k[q] <= cap, (q, k[q])
    assert case[0] == 1 or min(k["beta"], k["nominal"], k["M"]) > 0.05          # a K_ref of 0 would make "10 x K_ref" an exactness test


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the budget discriminates
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _yardstick(case):
    pr = P.problem(*case)
    b_ld, A_b = P.beta(pr["Kinv"], pr["Y"])
    b64 = R.to_f64(P.beta(pr["Kinv"], pr["Y"], np.float64)[0])
    M_ld, A_M = P.weights(pr["X"], pr["Kinv"], b64, pr["lam"], pr["sf"])
    return b_ld, A_b, b64, M_ld, A_M


def _band_term(Kinv, Y, b):
    """(a, i, j) of the largest term of a beta row that the 1e-9 band still passes when dropped, or None."""
    T = Kinv * Y.T[:, None, :]
    band = 1e-9 * np.abs(b) + 1e-9 * np.abs(b).max(axis=1, keepdims=True)
    ok = np.abs(T) <= band[:, :, None]
    if not ok.any():
        return None
    return np.unravel_index(np.argmax(np.where(ok, np.abs(T), -1.0)), T.shape)


def _defective_build(pr, defect, b64=None):
    """(beta (ds, N), M (ds, N, N) with element (i, j) at [a, i, j]) of a float64 build with ``defect``; None where it does not apply."""
    X, Y, Kinv, lam, sf = (np.asarray(pr[k]) for k in ("X", "Y", "Kinv", "lam", "sf"))
    ds, n = Y.shape[1], len(X)
    if b64 is None:
        b64 = R.to_f64(P.beta(Kinv, Y, np.float64)[0])
    b, Kw, emap = b64, Kinv, None
    if defect == "beta from K^T y":
        b = R.to_f64(P.beta(Kinv.transpose(0, 2, 1), Y, np.float64)[0])
    elif defect == "one beta term dropped":
        pick = _band_term(Kinv, Y, b64)
        if pick is None:
            return None
        b = b64.copy()
        b[pick[0], pick[1]] -= Kinv[pick] * Y[pick[2], pick[0]]
    elif defect == "weight from K_ij alone":                               # a symmetric matrix whose (i <= j) entries are K_ij
        Kw = np.triu(Kinv) + np.triu(Kinv, 1).transpose(0, 2, 1)
    elif defect == "weight from K_ji alone":
        Kw = np.tril(Kinv) + np.tril(Kinv, -1).transpose(0, 2, 1)
    elif defect == "lambda of GP 0 for every GP":
        if ds < 2 or all(np.array_equal(lam[a], lam[0]) for a in range(ds)):
            return None
        lam = np.tile(lam[:1], (ds, 1))
    elif defect == "exponent rounded to float32":
        emap = lambda e: e.astype(np.float32).astype(np.float64)  # noqa: E731
    if n == 1 and defect in ("beta from K^T y", "weight from K_ij alone", "weight from K_ji alone", "weight stored at the transposed place",
                              "exponent rounded to float32"):
        return None                                                       # one point: nothing to transpose, and its exponent is 0
    # (a beta defect is judged on beta: the weights take beta as given, on both sides)
    M = R.to_f64(P.weights(X, Kw, b64, lam, sf, np.float64, exponent_map=emap)[0])
    if defect == "sigma_f^2 for sigma_f^4":
        M = M / (sf * sf)[:, None, None]
    if defect == "weight stored at the transposed place":
        M = M.transpose(0, 2, 1)
    return b, M


def _present_band_passes(z, b, M):
    """The assertions of tests/test_gpu_parity.py::test_pack_constants on (beta, M with element (i, j) at [a, i, j])."""
    N, ds = z["X"].shape[0], z["Y"].shape[1]
    ok = True
    for a in range(ds):
        b_ref = z["Ky_inv"][a] @ z["Y"][:, a]
        ok &= np.allclose(b[a], b_ref, rtol=1e-9, atol=1e-9 * np.abs(b_ref).max())
        d = z["X"][:, None, :] - z["X"][None, :, :]
        lam_part = np.exp(-0.25 * np.sum(d * d / z["lambdas"][a], axis=2))
        Wsym = 0.5 * (z["Ky_inv"][a] + z["Ky_inv"][a].T) - np.outer(b_ref, b_ref)
        Mr = Wsym * lam_part * z["sigma_f"][a] ** 4
        ref = np.triu(Mr, 1) * 2 + np.diag(np.diag(Mr))
        ok &= np.allclose(M[a], ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max())
        ok &= bool(np.all(np.tril(M[a], -1) == 0))
    return bool(ok)


def _budget(case, b, M):
    """(K_beta, K_M, passes) of the new assertion on a ladder case: K <= min(10 K_ref, cap) on every entry, zeros below the diagonal."""
    b_ld, A_b, b64, M_ld, A_M = _yardstick(case)
    ds, n = b.shape
    kb, km = P.k_of(b, b_ld, A_b), P.k_of(M, M_ld, A_M, P.upper_mask(ds, n))
    kref = P.k_ref(*case)
    zeros = all(np.all(np.tril(M[a], -1) == 0) for a in range(ds))
    return kb, km, kb <= P.budget("beta", kref) and km <= P.budget("M", kref) and zeros


def test_the_clean_float64_build_passes_the_present_band_and_its_k_is_k_ref(golden):
    """The emulation without a defect: the present band passes it on g3, and on the ladder its K is K_ref itself -- inside 10 K_ref by
    construction; the absolute caps are sized on the HIP kernels, whose strided wave sums are shorter than a BLAS dot product, and an
    honest float64 beta may sit above them (printed)."""
    z = golden("g3_rollout_c1.npz")
    g3 = {"X": z["X"], "Y": z["Y"], "Kinv": z["Ky_inv"], "lam": z["lambdas"], "sf": z["sigma_f"]}
    assert _present_band_passes(z, *_defective_build(g3, None))
    over = []
    for case in CASES:
        kb, km, _ = _budget(case, *_defective_build(P.problem(*case), None, _yardstick(case)[2]))
        kref = P.k_ref(*case)
        assert kb == kref["beta"] and km == kref["M"], (case, kb, km)
        over += [(P.case_id(case), q, v) for q, v in (("beta", kb), ("M", km)) if v > P.CAP_K[q]]
    print("  plain float64 above the caps of the HIP path: %s" % (over or "nowhere"))


@pytest.mark.parametrize("defect", DEFECTS)
def test_budget_sees_what_the_present_band_does_not(golden, defect):
    z = golden("g3_rollout_c1.npz")
    g3 = {"X": z["X"], "Y": z["Y"], "Kinv": z["Ky_inv"], "lam": z["lambdas"], "sf": z["sigma_f"]}
    assert np.all(z["sigma_f"] == 1.0) and np.abs(z["Ky_inv"] - z["Ky_inv"].transpose(0, 2, 1)).max() < 1e-11 * np.abs(z["Ky_inv"]).max()
    on_g3 = _defective_build(g3, defect)                                   # (None: the band passes no dropped term of g3 at all)
    old_passes = on_g3 is not None and _present_band_passes(z, *on_g3)
    ks, missed = [], []
    for case in CASES:
        out = _defective_build(P.problem(*case), defect, _yardstick(case)[2])
        if out is None:
            continue
        kb, km, ok = _budget(case, *out)
        ks.append(max(kb, km))
        if ok:
            missed.append((P.case_id(case), kb, km))
    print("DEFECT %-40s present band on g3: %s | new budget on %2d ladder cases: worst K %.3g ... %.3g, passes on %d"
          % (defect + ":", "passes" if old_passes else "CATCHES it", len(ks), min(ks), max(ks), len(missed)))
    assert old_passes == (defect not in OLD_BAND_CATCHES), defect
    if defect == "one beta term dropped":
        T = np.abs(z["Ky_inv"] * z["Y"].T[:, None, :])
        b = np.abs(np.einsum("aij,ja->ai", z["Ky_inv"], z["Y"]))
        print("       (the smallest term of a g3 row is %.3g of what the band allows its row: it passes no dropped term there)"
              % (T / (1e-9 * b + 1e-9 * b.max(axis=1, keepdims=True))[:, :, None]).min())
    assert len(ks) >= (1 if defect == "one beta term dropped" else 5) and not missed, missed
