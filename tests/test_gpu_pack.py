"""Every entry of the PACK BUILD (gpmpc_pack_build, gpmpc_pack_build_strided, gpmpc_pack_build_beta, the nominal-residual build,
gpmpc_pack_resize + build) against the extended-precision restatement of tests/pack_reference.py, on EVERY entry of the export: beta from
targets in the row form K y, the weights M(i <= j) = w (1/2 (K_ij + K_ji) - beta_i beta_j) sf^4 exp(-e), exact zeros below the diagonal and
in every padded row and column.  The inputs are what the one direct test of the build (tests/test_gpu_parity.py::test_pack_constants: N = 100,
sigma_f = 1, symmetric Ky_inv, a 1e-9 band) cannot see through: amplitudes off 1, a Ky_inv that is NON-symmetric by 1e-3 (as kinv_append /
kinv_remove / gp_replace leave it), distinct lambdas per GP, and a ladder of sizes with one point either side of every 32-tile, 64-pad and
256-thread edge of k_pack_weights / k_pack_beta / k_pack_residual (tests/pack_reference.py::LADDER_N; D = 1 ... 8, ds = 1 ... 8).

The statistic is K = max |HIP - reference| / (2^-53 A) with the units of tests/pack_reference.py: A_beta = sum_j |Kinv_ij y_j|, for a nominal
pack sum_j |Kinv_ij| rho_j, A_M = w sf^4 exp(-e) [|ksym| + |beta_i beta_j| + |ksym - beta_i beta_j| (1 + e)].  The weights are judged with
the float64 beta the pack exported taken as given, so the two links are judged apart (the convention of tests/test_gpu_accuracy.py).

Asserted on every case: K <= 10 K_ref of the SAME case, K_ref being the plain float64 numpy evaluation of the same formulas
(tests/pack_reference.py::k_ref; tests/test_host_pack.py records it: beta 0.35 ... 4.8, nominal beta 0.24 ... 3.8, M 0.10 ... 3.0, and shows
which defects this budget sees and the 1e-9 band does not), and the absolute caps of tests/pack_reference.py::CAP_K per unit.

Measured on an MI355X, worst K over the cases of an entry point (the K_ref of the same cases, as that machine's numpy gave them, in brackets):
    gpmpc_pack_build, ladder of 18 sizes      beta 0.35 ... 2.14 (0.35 ... 4.71)      M 0.10 ... 2.86 (0.10 ... 3.13)
        largest K / K_ref on one case         beta 1.7 (N = 2: 0.955 | 0.556)         M 1.25 (N = 300: 2.19 | 1.75)
    far clusters (weights that underflow)     beta 1.57 (1.44)                        M 1.28 (1.25)
    strided: view, stack, one K (abi / view / contiguous 2-D): bit-equal to the packed builds of the same data, which give
        one matrix per GP                     beta 1.82                               M 2.86
        one matrix for all GPs                beta 2.12                               M 2.85
    gpmpc_pack_build_beta                     (beta given: copied bit for bit)        M 2.87
    nominal-residual build (two models)       nominal beta 2.10 (1.37 ... 3.80)       M 2.78
    gpmpc_pack_resize + build (70 | 120)      beta 0.98                               M 2.17
No entry lies more than a factor 1.7 above K_ref on the same case.  Against what one might expect of a GPU sum, beta sits BELOW K_ref from
N = 32 on (N = 520: 0.76 against 4.1): k_pack_beta gives each of 64 lanes a chain of ceil(N / 64) fused multiply-adds and joins them in a
6-level butterfly, at most 9 + 6 roundings deep at N = 520, where numpy's dot product runs chains several times as long; at N <= 2 the one
or two fmas differ from numpy's multiply and add by a rounding (0.955 against 0.556).  The weights follow K_ref within 25 %: the same
elementwise operations, sf^4 formed as (sf^2)^2 and the device's exp.
The caps (tests/pack_reference.py::CAP_K), twice the worst measured value rounded up to two digits: beta 4.3, nominal beta 4.2, M 5.8.

Checked once on scratch copies of csrc/pack_build.hip (not committed): `kij` for `0.5 * (kij + kji)`, `sf2` for `sf4`, and `j * ld + row` for
`row * ld + j` in k_pack_beta each make this module fail while test_pack_constants still passes.
"""
import ctypes

import numpy as np
import pytest
import torch

import gpstate_reference as R
import pack_reference as P

pytestmark = pytest.mark.gpu

E_ARG = -1
CASES = P.ladder()
IDS = [P.case_id(c) for c in CASES]
SOME = [c for c in CASES if c[0] in (2, 33, 129, 257)]                      # ds = 2, 5, 3, 4: every stride has something to separate
SOME_IDS = [P.case_id(c) for c in SOME]
NOMINAL = [c for c in CASES if c[0] in (33, 65, 300)]
SPREAD = 400.0
_WORST = {}
_REFS = {}


@pytest.fixture(scope="module")
def G():
    import gaussian_process_mpc_amd as g
    g.require_gpu()
    yield g
    print("\n  worst K per entry point and unit: " + ", ".join("%s %s %.3g" % (k[0], k[1], v) for k, v in sorted(_WORST.items())))


def _L():
    from gaussian_process_mpc_amd._lib import lib
    return lib()


def _sp():
    from gaussian_process_mpc_amd._lib import stream_ptr
    return stream_ptr()


def _check(rc, what):
    from gaussian_process_mpc_amd._lib import check
    check(rc, what)


def _hp(a):
    from gaussian_process_mpc_amd._lib import host_doubles
    return host_doubles(np.array(a))[1]


def _dev(a):
    return torch.tensor(np.array(a, dtype=np.float64, order="C"), device="cuda")


def _vp(t):
    assert t is None or (t.is_contiguous() and t.dtype == torch.float64)
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same(a, b):
    """Bit for bit, numpy."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


class _Pack:
    """A pack handle of the C ABI, destroyed on exit."""

    def __init__(self, pr, n=None):
        self.ds, self.da, self.n = pr["ds"], pr["da"], pr["n"] if n is None else n
        self.Np = (self.n + 63) // 64 * 64
        self.h = ctypes.c_void_p()
        _check(_L().gpmpc_pack_create(ctypes.byref(self.h), self.n, self.ds, self.da), "gpmpc_pack_create")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        _L().gpmpc_pack_destroy(self.h)
        self.h = None

    def build(self, pr, Kinv="packed", ld=None, gstride=None, beta_src=None, lam=None, expect=0):
        """gpmpc_pack_build on the packed Ky_inv of `pr`, gpmpc_pack_build_strided on the device buffer `Kinv` when a leading dimension is
        given, gpmpc_pack_build_beta when `beta_src` [N][ds] is (Kinv None: NULL).  Returns the return code (asserted to be `expect`)."""
        X, Y = _dev(pr["X"]), _dev(pr["Y"])
        lp, sp = _hp(pr["lam"] if lam is None else lam), _hp(pr["sf"])
        if isinstance(Kinv, str):
            Kinv = _dev(pr["Kinv"] if pr["Kinv"].ndim == 3 else np.broadcast_to(pr["Kinv"], (self.ds,) + pr["Kinv"].shape))
        if beta_src is not None:
            rc = _L().gpmpc_pack_build_beta(self.h, _vp(X), _vp(beta_src), _vp(Kinv), lp, sp, _sp())
        elif ld is not None:
            rc = _L().gpmpc_pack_build_strided(self.h, _vp(X), _vp(Y), _vp(Kinv), ld, gstride, lp, sp, _sp())
        else:
            rc = _L().gpmpc_pack_build(self.h, _vp(X), _vp(Y), _vp(Kinv), lp, sp, _sp())
        torch.cuda.synchronize()
        assert rc == expect, rc
        return rc

    def export(self):
        return _export(self.h, self.Np, self.ds)


def _export(h, Np, ds):
    """(beta (ds, Np), weights (ds, Np, Np)) as the pack holds them, padding included; the buffers are NaN before the call."""
    b, w = _nan(ds, Np), _nan(ds, Np, Np)
    _check(_L().gpmpc_pack_export(h, _vp(b), _vp(w), _sp()), "gpmpc_pack_export")
    torch.cuda.synchronize()
    return b.cpu().numpy(), w.cpu().numpy()


def _gppack(G, pr, Kinv="own", Y=None, **kw):
    """GPPack on (writable copies of) a problem's arrays; `Kinv`: a device tensor / view to read instead of the problem's own."""
    K = np.array(pr["Kinv"]) if isinstance(Kinv, str) else Kinv
    return G.GPPack(np.array(pr["X"]), np.array(pr["Y"] if Y is None else Y), K, np.array(pr["lam"]), np.array(pr["sf"]), **kw)


def _judge(entry, pr, kref, beta, W, nominal=None, beta_given=False):
    """Every entry of an export against the reference.  Prints the figures, then asserts: exact zeros in the padding and below the
    diagonal, 0 where the reference weight underflows, K <= 10 K_ref and the caps on beta (unless it was given) and on M."""
    n, ds = pr["n"], pr["ds"]
    Np = (n + 63) // 64 * 64
    assert beta.shape == (ds, Np) and W.shape == (ds, Np, Np)
    got = W[:, :n, :n].transpose(0, 2, 1)                                   # element (i, j) is stored at [a, j, i]
    key = (id(pr), None if nominal is None else nominal[0].tobytes(), beta[:, :n].tobytes())
    if key not in _REFS:                                                    # one reference per distinct (inputs, exported beta): bit-equal builds share it
        if nominal is None:
            b_ref = P.beta(pr["Kinv"], pr["Y"])
        else:
            b_ref = P.beta_nominal(pr["Kinv"], pr["X"], pr["Y"], nominal[0], nominal[1])
        _REFS[key] = (b_ref, P.weights(pr["X"], pr["Kinv"], beta[:, :n], pr["lam"], pr["sf"]))
    (b_ref, b_unit), (M_ref, A_M) = _REFS[key]
    mask = P.upper_mask(ds, n)
    k = {"M": P.k_of(got, M_ref, A_M, mask)}
    unit = "nominal" if nominal is not None else "beta"
    if not beta_given:
        k[unit] = P.k_of(beta[:, :n], b_ref, b_unit)
    print("  PACK %-22s %s: " % (entry, P.case_id((n, pr["D"], ds, False))) + "  ".join("K_%s %.3g (K_ref %.3g)" % (q, v, kref[q]) for q, v in sorted(k.items())))
    assert np.all(beta[:, n:] == 0), "beta: padded rows"
    assert np.all(W[:, n:, :] == 0) and np.all(W[:, :, n:] == 0), "weights: padded rows / columns"
    assert np.all(got[~mask] == 0), "weights: below the diagonal"
    under = mask & (np.asarray(M_ref) == 0)
    assert np.all(got[under] == 0), "weights: the reference underflows to 0"
    bad = []
    for q, v in k.items():
        _WORST[(entry, q)] = max(_WORST.get((entry, q), 0.0), v) if v == v else float("nan")
        if not v <= P.EXCESS_FACTOR * kref[q]:
            bad.append((q, v, "10 x K_ref", P.EXCESS_FACTOR * kref[q]))
        if not v <= P.CAP_K[q]:
            bad.append((q, v, "cap", P.CAP_K[q]))
    assert not bad, bad
    return k


# ------------------------------------------------------------------------------------------------------------------------------
# the ladder: gpmpc_pack_build, and GPPack on the same data
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pack_build_on_the_ladder(G, case):
    pr = P.problem(*case)
    with _Pack(pr) as pk:
        pk.build(pr)
        beta, W = pk.export()
    _judge("build", pr, P.k_ref(*case), beta, W)
    pack = _gppack(G, pr)
    b2, W2 = _export(pack.handle, pack.Np, pack.ds)
    assert _same(beta, b2) and _same(W, W2)
    assert pack.shared_lambda == (case[3] and 1 <= pr["da"] <= 2)            # (the one-lambda kernels exist for one or two inputs)


def test_weights_between_far_clusters_underflow_to_zero(G):
    """Two clusters 400 apart: e > 15000 between them, exp underflows in float64 AND in long double -- the export must be exactly 0 there
    (and inside the budget within the clusters)."""
    n, D, ds = 33, 2, 2
    pr = P.problem(n, D, ds, spread=SPREAD)
    with _Pack(pr) as pk:
        pk.build(pr)
        beta, W = pk.export()
    _judge("build far clusters", pr, P.k_ref(n, D, ds, spread=SPREAD), beta, W)
    got = W[:, :n, :n].transpose(0, 2, 1)
    h = n // 2
    assert np.all(got[:, :h, h:] == 0) and np.abs(got[:, :h, :h][P.upper_mask(ds, h)]).min() > 0
    if R.HAVE_LD:
        M_ref = _REFS[(id(pr), None, beta[:, :n].tobytes())][1][0]
        assert np.all(np.asarray(M_ref)[:, :h, h:] == 0)           # the check above was not vacuous


# ------------------------------------------------------------------------------------------------------------------------------
# strided builds
# ------------------------------------------------------------------------------------------------------------------------------
def _padded_stack(K, ld, gstride):
    """The matrices K (g, n, n) at row stride `ld` and matrix stride `gstride` in a flat NaN buffer (with NaN behind the last row too)."""
    g, n, _ = K.shape
    flat = _nan(max(g - 1, 0) * gstride + ld * n + 3)
    for a in range(g):
        flat[a * gstride:a * gstride + ld * n].view(n, ld)[:, :n] = _dev(K[a])
    return flat


@pytest.mark.parametrize("case", SOME, ids=SOME_IDS)
def test_strided_builds(G, case):
    """Each strided form holds the budget, equals the packed build of the same data bit for bit, and leaves its input -- NaN padding
    included -- untouched.  A read past N (row or column) would turn the result NaN."""
    n, D, ds, shared = case
    pr, pr1 = P.problem(*case), P.problem(*case, one_matrix=True)
    kref, kref1 = P.k_ref(*case), P.k_ref(*case, one_matrix=True)
    with _Pack(pr) as pk:
        pk.build(pr)
        packed = pk.export()
        pk.build(pr1)                                                        # one matrix, expanded to a packed [ds][N][N]
        packed1 = pk.export()
    _judge("build (packed)", pr, kref, *packed)
    _judge("build (packed, one K)", pr1, kref1, *packed1)
    assert not _same(packed[0], packed1[0])

    def through_gppack(pr_, Kt):
        pack = _gppack(G, pr_, Kt)
        return _export(pack.handle, pack.Np, pack.ds)

    def through_abi(pr_, flat, ld, gstride):
        with _Pack(pr_) as pk:
            pk.build(pr_, Kinv=flat, ld=ld, gstride=gstride)
            return pk.export()

    cap = n + 7
    variants = []
    # a view of a capacity-padded buffer whose padding is NaN (GPPack reads it in place: ld = cap, gstride = cap^2)
    buf = _nan(ds, cap, cap)
    buf[:, :n, :n] = _dev(pr["Kinv"])
    assert not buf[:, :n, :n].is_contiguous()
    variants.append(("strided view", pr, kref, packed, buf, lambda: through_gppack(pr, buf[:, :n, :n])))
    # a 3-D stack whose matrix stride is not ld * N
    ld, gs = n + 3, (n + 3) * n + 5
    flat = _padded_stack(pr["Kinv"], ld, gs)
    variants.append(("strided stack", pr, kref, packed, flat, lambda: through_abi(pr, flat, ld, gs)))
    # one matrix shared by all GPs (gstride = 0): padded through the ABI, padded and contiguous through GPPack
    flat1 = _padded_stack(pr1["Kinv"][None], ld, 0)
    variants.append(("strided one K abi", pr1, kref1, packed1, flat1, lambda: through_abi(pr1, flat1, ld, 0)))
    buf1 = _nan(cap, cap)
    buf1[:n, :n] = _dev(pr1["Kinv"])
    variants.append(("strided one K view", pr1, kref1, packed1, buf1, lambda: through_gppack(pr1, buf1[:n, :n])))
    cont1 = _dev(pr1["Kinv"])
    variants.append(("strided one K 2-D", pr1, kref1, packed1, cont1, lambda: through_gppack(pr1, cont1)))
    for name, pr_, kref_, ref, src, run in variants:
        before = src.clone()
        beta, W = run()
        assert torch.equal(_bits(src), _bits(before)), name                 # the input, NaN padding included, bitwise unchanged
        assert not np.isnan(beta).any() and not np.isnan(W).any(), name
        _judge(name, pr_, kref_, beta, W)
        assert _same(beta, ref[0]) and _same(W, ref[1]), name


# ------------------------------------------------------------------------------------------------------------------------------
# gpmpc_pack_build_beta
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SOME, ids=SOME_IDS)
def test_build_beta(G, case):
    """beta handed over: copied bit for bit into [ds][Np] and zero padded; with Ky_inv the weights meet the budget with THAT beta, with
    Ky_inv = NULL every weight is exactly 0.  GPPack(y_is_beta=True) -- packed, and from a strided view, which it makes contiguous -- agrees."""
    n, D, ds, shared = case
    pr = P.problem(*case)
    kref = P.k_ref(*case)
    src = np.ascontiguousarray(R.to_f64(P.beta(pr["Kinv"], pr["Y"], np.float64)[0]).T) * 1.25      # [N][ds]; not what K y gives
    src_dev = _dev(src)
    with _Pack(pr) as pk:
        pk.build(pr, beta_src=src_dev)
        beta, W = pk.export()
        pk.build(pr, Kinv=None, beta_src=src_dev)
        beta0, W0 = pk.export()
    assert _same(beta[:, :n], np.ascontiguousarray(src.T)) and _same(beta0, beta)
    _judge("build_beta", pr, kref, beta, W, beta_given=True)
    assert np.all(beta0[:, n:] == 0) and np.all(W0 == 0) and not np.signbit(W0).any()
    assert np.array_equal(src_dev.cpu().numpy(), src)
    pack = _gppack(G, pr, Y=src, y_is_beta=True)
    b2, W2 = _export(pack.handle, pack.Np, ds)
    assert _same(b2, beta) and _same(W2, W)
    buf = _nan(ds, n + 7, n + 7)
    buf[:, :n, :n] = _dev(pr["Kinv"])
    pack = _gppack(G, pr, buf[:, :n, :n], Y=src, y_is_beta=True)
    b3, W3 = _export(pack.handle, pack.Np, ds)
    assert _same(b3, beta) and _same(W3, W)
    pack = _gppack(G, pr, None, Y=src, y_is_beta=True)
    b4, W4 = _export(pack.handle, pack.Np, ds)
    assert _same(b4, beta) and np.all(W4 == 0)


# ------------------------------------------------------------------------------------------------------------------------------
# nominal model: beta from residual targets (k_pack_residual)
# ------------------------------------------------------------------------------------------------------------------------------
def _set_nominal(pk, W, c):
    _check(_L().gpmpc_pack_set_nominal(pk.h, None if W is None else _hp(W), None if c is None else _hp(c), _sp()), "gpmpc_pack_set_nominal")


@pytest.mark.parametrize("case", NOMINAL, ids=[P.case_id(c) for c in NOMINAL])
def test_nominal_residual_build(G, case):
    """beta = Kinv (y - X W^T - c) in its own unit sum_j |Kinv_ij| rho_j, the weights with that beta; a new model followed by a build
    gives the new beta; clearing the model restores the plain beta bit for bit."""
    pr = P.problem(*case)
    kref = P.k_ref(*case)
    W1, c1 = np.array(pr["W"]), np.array(pr["c"])
    W2, c2 = np.ascontiguousarray(-0.5 * W1[:, ::-1]), c1 + 0.7
    with _Pack(pr) as pk:
        pk.build(pr)
        plain = pk.export()
        _set_nominal(pk, W1, c1)
        assert _L().gpmpc_pack_export(pk.h, None, None, _sp()) == -5          # not built until the next build
        pk.build(pr)
        first = pk.export()
        _set_nominal(pk, W2, c2)
        pk.build(pr)
        second = pk.export()
        _set_nominal(pk, None, None)
        pk.build(pr)
        cleared = pk.export()
    _judge("build", pr, kref, *plain)
    _judge("nominal build", pr, kref, *first, nominal=(W1, c1))
    _judge("nominal build", pr, kref, *second, nominal=(W2, c2))
    b1_ref, unit = P.beta_nominal(pr["Kinv"], pr["X"], pr["Y"], W1, c1)
    assert P.k_of(second[0][:, :pr["n"]], b1_ref, unit) > 1e6                 # the second model is another model
    assert _same(cleared[0], plain[0]) and _same(cleared[1], plain[1])
    pack = _gppack(G, pr, nominal=(W1, c1))
    b, Wt = _export(pack.handle, pack.Np, pack.ds)
    assert _same(b, first[0]) and _same(Wt, first[1])


# ------------------------------------------------------------------------------------------------------------------------------
# resize into the same padded size
# ------------------------------------------------------------------------------------------------------------------------------
RESIZE_D, RESIZE_DS = 3, 2


def _rollouts(G, pack, full):
    """Rollouts of B = 1 and B = 4, H = 2, with gradient, under the default plan: a list of numpy arrays."""
    ds, da = pack.ds, pack.da
    rng = np.random.default_rng(5)
    cost = G.CostParams(-1.0, 0.01 * np.eye(ds), 0.001 * np.eye(da))
    out = []
    for B in (1, 4):
        x0, U = rng.uniform(-0.5, 0.5, (B, ds)), rng.uniform(-0.5, 0.5, (B, 2, da))
        r = G.rollout(pack, x0, U, cost, want_grad=True)
        out += [r[k].cpu().numpy().copy() for k in ("cost", "grad", "means", "vars")]
        if full:
            r = G.rollout_fullcov(pack, x0, U, cost, want_grad=True)
            out += [r[k].cpu().numpy().copy() for k in ("cost", "grad", "means", "covs")]
    assert all(np.isfinite(a).all() for a in out)
    return out


@pytest.mark.parametrize("full", [False, True], ids=["diagonal", "fullcov"])
def test_resize_into_the_same_padded_size(G, full):
    """120 -> 70 -> 120 points in one pack (Np = 128 throughout): after each refill the exports equal those of a freshly created pack of
    that size bit for bit, every stale row and column is exactly 0, and the rollouts (with enable_fullcov(): the full-covariance ones too,
    whose cross weights follow every build) agree bit for bit."""
    big, small = P.problem(120, RESIZE_D, RESIZE_DS), P.problem(70, RESIZE_D, RESIZE_DS)

    def fresh(pr):
        p = _gppack(G, pr)
        return p.enable_fullcov() if full else p

    pack = fresh(big)
    handle = pack.handle.value
    for step, pr in (("120 -> 70", small), ("70 -> 120", big)):
        assert pack.rebuild(_dev(pr["X"]), _dev(pr["Y"]), _dev(pr["Kinv"]), np.array(pr["lam"]), np.array(pr["sf"])) and pack.handle.value == handle
        n = ctypes.c_int()
        _L().gpmpc_pack_dims(pack.handle, ctypes.byref(n), None, None, None)
        assert n.value == pr["n"] and pack.Np == 128
        beta, W = _export(pack.handle, 128, RESIZE_DS)
        _judge("resize + build", pr, P.k_ref(pr["n"], RESIZE_D, RESIZE_DS), beta, W)           # (stale rows and columns: its zero checks)
        other = fresh(pr)
        b2, W2 = _export(other.handle, 128, RESIZE_DS)
        assert _same(beta, b2) and _same(W, W2), step
        for a, b in zip(_rollouts(G, pack, full), _rollouts(G, other, full)):
            assert _same(a, b), step
    # the C entry itself: another padded size is refused and leaves the pack as it was
    assert _L().gpmpc_pack_resize(pack.handle, 129) == E_ARG and _L().gpmpc_pack_resize(pack.handle, 0) == E_ARG
    b3, W3 = _export(pack.handle, 128, RESIZE_DS)
    assert _same(b3, beta) and _same(W3, W)


# ------------------------------------------------------------------------------------------------------------------------------
# lifecycle order
# ------------------------------------------------------------------------------------------------------------------------------
def _fullcov_rollout(G, pack):
    """(cost, grad, means, covs) of one full-covariance rollout, B = 2, H = 3."""
    rng = np.random.default_rng(11)
    cost = G.CostParams(-1.0, 0.01 * np.eye(pack.ds), 0.001 * np.eye(pack.da))
    r = G.rollout_fullcov(pack, rng.uniform(-0.5, 0.5, (2, pack.ds)), rng.uniform(-0.5, 0.5, (2, 3, pack.da)), cost, want_grad=True)
    torch.cuda.synchronize()
    assert all(torch.isfinite(r[k]).all() for k in r)
    return [r[k].clone() for k in ("cost", "grad", "means", "covs")]


@pytest.mark.parametrize("D,ds,shared", [(3, 2, True), (4, 3, False)], ids=["one-lambda", "distinct-no-tables"])
def test_fullcov_rollout_does_not_depend_on_the_order_of_build_and_enable(G, monkeypatch, D, ds, shared):
    """N = 100 (Np = 128), da = 1: the full-covariance rollout after (a) build, then enable_fullcov, (b) enable_fullcov on a fresh pack, then
    the build, (c) as (a), then a rebuild for 101 points and one back to the 100: bit for bit the same.  GPMPC_FC_SHARED=1 (read at pack
    creation) makes the one-lambda pack run its cross unit through pair_kernel_sbfx.h at this small size -- the default plan takes that path
    from B Np^2 pairs >= 3.5e7 --, i.e. from the one-lambda tables of the pack's index data and the column rows that (a) enable_fullcov,
    (b) the first build, (c) the first enable_fullcov allocates and every later build refreshes; the plan of EACH pack is asserted to say so,
    so that a table or an allocation that is missing cannot pass as a quiet change of path.  ds = 3 with distinct lambdas has neither and must
    plan the per-unit kernels.  (The commit before the index data became one allocation, dcfe28d, showed the same equality in all three
    orders under the same forced plan, and the same bits.)"""
    monkeypatch.setenv("GPMPC_FC_SHARED", "1")
    pr, other = P.problem(100, D, ds, shared=shared), P.problem(101, D, ds, shared=shared)
    first = _gppack(G, pr, fullcov=True)
    assert first.fullcov
    back = _gppack(G, pr).enable_fullcov()
    for q in (other, pr):
        assert back.rebuild(_dev(q["X"]), _dev(q["Y"]), _dev(q["Kinv"]), np.array(q["lam"]), np.array(q["sf"]))
    out = []
    for pack in (_gppack(G, pr).enable_fullcov(), first, back):
        plan = pack.plan_fullcov(2, 3)
        assert plan["shared_cross_units"] == (1 if shared else 0), plan
        out.append(_fullcov_rollout(G, pack))
    for name, x, y, z in zip(("cost", "grad", "means", "covs"), *out):
        assert torch.equal(x, y), ("enable before the first build", name)
        assert torch.equal(x, z), ("101 points and back", name)


# ------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_refused_builds_leave_the_pack_as_it_was(G):
    pr = P.problem(70, RESIZE_D, RESIZE_DS)
    n, ds = pr["n"], pr["ds"]
    pack = _gppack(G, pr)
    before = _export(pack.handle, pack.Np, ds)
    rolls = _rollouts(G, pack, False)
    X, Y, K = _dev(pr["X"]), _dev(pr["Y"]), _dev(pr["Kinv"])
    sp = _hp(pr["sf"])

    def lam_with(a, k, v):
        lam = np.array(pr["lam"])
        lam[a, k] = v
        return _hp(lam)

    L = _L()
    refusals = {
        "lambda = 0 in the last GP": lambda: L.gpmpc_pack_build(pack.handle, _vp(X), _vp(Y), _vp(K), lam_with(ds - 1, RESIZE_D - 1, 0.0), sp, _sp()),
        "lambda < 0 in the last GP": lambda: L.gpmpc_pack_build(pack.handle, _vp(X), _vp(Y), _vp(K), lam_with(ds - 1, RESIZE_D - 1, -1.5), sp, _sp()),
        "a NaN lambda": lambda: L.gpmpc_pack_build(pack.handle, _vp(X), _vp(Y), _vp(K), lam_with(0, 1, float("nan")), sp, _sp()),
        "a NaN lambda (build_beta)": lambda: L.gpmpc_pack_build_beta(pack.handle, _vp(X), _vp(Y), _vp(K), lam_with(0, 1, float("nan")), sp, _sp()),
        "ld < N": lambda: L.gpmpc_pack_build_strided(pack.handle, _vp(X), _vp(Y), _vp(K), n - 1, n * n, _hp(pr["lam"]), sp, _sp()),
        "ld = 0": lambda: L.gpmpc_pack_build_strided(pack.handle, _vp(X), _vp(Y), _vp(K), 0, n * n, _hp(pr["lam"]), sp, _sp()),
        "NULL Ky_inv with targets": lambda: L.gpmpc_pack_build(pack.handle, _vp(X), _vp(Y), None, _hp(pr["lam"]), sp, _sp()),
        "NULL Ky_inv (strided)": lambda: L.gpmpc_pack_build_strided(pack.handle, _vp(X), _vp(Y), None, n, n * n, _hp(pr["lam"]), sp, _sp()),
    }
    for what, call in refusals.items():
        assert call() == E_ARG, what
        torch.cuda.synchronize()
        after = _export(pack.handle, pack.Np, ds)
        assert _same(after[0], before[0]) and _same(after[1], before[1]), what
        for a, b in zip(_rollouts(G, pack, False), rolls):
            assert _same(a, b), what
