"""CPU-only tests of the linear nominal model: the two C ABI entry points are exported, declared and check their arguments before any
device call; LinearNominalModel; the pack key and the warning of Dynamics; and the float64 reference helper of the GPU tests
(tests/nominal_reference.py) against Gauss-Hermite quadrature of the GP posterior."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpmpc_pack_set_nominal", "gpmpc_pack_get_nominal")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import gaussian_process_mpc_amd as g
    return g


def test_nominal_symbols_are_exported_and_declared(built):
    from gaussian_process_mpc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gpmpc_[a-z_]+)\s*\(", hdr))
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(h, name) is not None
        assert getattr(built.lib(), name).argtypes == _lib.SIGNATURES[name][1]


def test_nominal_argument_validation_without_device(built):
    lib = built.lib()
    w = (ctypes.c_double * 6)(*([0.0] * 6))
    b = (ctypes.c_double * 2)(0.0, 0.0)
    assert lib.gpmpc_pack_set_nominal(None, None, None, None) == -1          # GPMPC_E_ARG: no pack
    assert lib.gpmpc_pack_set_nominal(None, w, b, None) == -1
    assert lib.gpmpc_pack_get_nominal(None, w, b) == -1
    assert lib.gpmpc_pack_get_nominal(None, None, None) == -1


def test_linear_nominal_model_call_and_identity(built):
    LinearNominalModel = built.LinearNominalModel
    m = LinearNominalModel([0.5, -2.0, 0.25], bias=0.125)
    X = torch.tensor([[1.0, 2.0, 4.0], [0.0, 1.0, -4.0], [2.0, 0.0, 0.0]], dtype=torch.float64)
    out = m(X)
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (3, 1) and out.dtype == torch.float64
    np.testing.assert_allclose(out.numpy().reshape(-1), [0.5 - 4.0 + 1.0 + 0.125, -2.0 - 1.0 + 0.125, 1.0 + 0.125], rtol=0, atol=1e-15)
    assert LinearNominalModel([1.0, 0.0])(X[:, :2]).shape == (3, 1)             # bias defaults to 0
    np.testing.assert_array_equal(LinearNominalModel([1.0, 0.0])(X[:, :2]).numpy().reshape(-1), X[:, 0].numpy())
    with pytest.raises(ValueError):
        m(X[:, :2])                                                             # wrong input dimension
    with pytest.raises(ValueError):
        LinearNominalModel([1.0, float("nan")])
    ident = LinearNominalModel.identity(3, 2)
    assert len(ident) == 3 and all(isinstance(q, LinearNominalModel) for q in ident)
    Z = torch.arange(20, dtype=torch.float64).reshape(4, 5)
    for a, q in enumerate(ident):
        assert q.bias == 0.0 and q.weights.shape == (5,)
        np.testing.assert_array_equal(q(Z).numpy().reshape(-1), Z[:, a].numpy())
    from gaussian_process_mpc_amd.nominal import stack_linear
    W, b = stack_linear(ident, 3, 2)
    np.testing.assert_array_equal(W, np.eye(5)[:3])
    np.testing.assert_array_equal(b, np.zeros(3))
    assert stack_linear([ident[0], lambda x: x[:, :1], ident[2]], 3, 2) is None
    assert stack_linear(None, 3, 2) is None


def _bare_dynamics(built, state_dim, action_dim, nominal_models):
    """A Dynamics without its GPs (they need a GPU): what the pack key and the warning depend on is host state only."""
    d = object.__new__(built.Dynamics)
    d.state_dim, d.action_dim, d.nominal_models = state_dim, action_dim, nominal_models
    d.gpr_err = []
    d._nominal_warned = False
    return d


def test_dynamics_pack_key_follows_the_nominal_models(built):
    LinearNominalModel, Dynamics = built.LinearNominalModel, built.Dynamics
    d = _bare_dynamics(built, 2, 1, LinearNominalModel.identity(2, 1))
    k0 = d._key()
    assert Dynamics._same_key(k0, d._key())
    d.nominal_models[1] = LinearNominalModel([0.0, 1.0, 0.0])                  # same coefficients, another object: same pack
    assert Dynamics._same_key(k0, d._key())
    d.nominal_models[1] = LinearNominalModel([0.0, 1.0, 0.05])
    assert not Dynamics._same_key(k0, d._key())
    d.nominal_models[1] = LinearNominalModel([0.0, 1.0, 0.0], bias=1e-3)
    assert not Dynamics._same_key(k0, d._key())
    plain = _bare_dynamics(built, 2, 1, None)
    assert not Dynamics._same_key(k0, plain._key()) and plain._key()[-1] is None
    W, b = d._linear_nominal()
    np.testing.assert_array_equal(W, [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    np.testing.assert_array_equal(b, [0.0, 1e-3])


def test_dynamics_warns_once_for_a_nonlinear_nominal_model(built):
    d = _bare_dynamics(built, 2, 1, [lambda x: torch.tanh(x[:, 0:1]), built.LinearNominalModel([0.0, 1.0, 0.0])])
    with pytest.warns(UserWarning, match="rollout ignores nominal models"):
        assert d._linear_nominal() is None
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert d._linear_nominal() is None                                       # said once
        assert d._key()[-1] is None
    with warnings.catch_warnings():                                               # linear models and no models: silent
        warnings.simplefilter("error")
        assert _bare_dynamics(built, 2, 1, built.LinearNominalModel.identity(2, 1))._linear_nominal() is not None
        assert _bare_dynamics(built, 2, 1, None)._linear_nominal() is None


def test_mpc_forwards_nominal_models_signature(built):
    import inspect
    sig = inspect.signature(built.RiskSensitiveMPC.__init__)
    assert "nominal_models" in sig.parameters and sig.parameters["nominal_models"].default is None
    sig = inspect.signature(built.GPPack.__init__)
    assert "nominal" in sig.parameters and sig.parameters["nominal"].default is None
    assert "nominal" in inspect.signature(built.GPPack.rebuild).parameters and isinstance(built.GPPack.nominal, property)


@pytest.mark.parametrize("case", [0, 1, 2])
def test_reference_helper_matches_quadrature(case):
    """The helper's step moments (oracle + autograd cross term) against 60 x 60 Gauss-Hermite quadrature of the GP posterior plus
    the linear model, 2-D input: 1e-9."""
    from oracle import gpmpc_oracle as O
    from nominal_reference import nominal_step, quadrature_moments
    rng = np.random.default_rng(77 + case)
    N = 40
    X = np.concatenate((rng.uniform(-2, 2, size=(N, 1)), rng.uniform(-1, 1, size=(N, 1))), axis=1)
    y = X[:, 0] + 0.1 * np.tanh(X[:, 0]) + 0.1 * X[:, 1]
    lam = rng.uniform(2.0, 6.0, size=2)
    sf, sn = [1.0, 1.3, 0.8][case], 1e-2
    n = np.array([[1.0, 0.05], [0.7, -0.3], [0.0, 0.0]][case])
    c = [0.01, -0.2, 0.0][case]
    u = np.array([[0.3, -0.4], [-0.8, 0.6], [0.1, 0.2]][case])
    s = np.array([[0.02, 1e-3], [0.2, 1e-3], [1e-3, 1e-3]][case])
    Ky_inv = O.kernel_matrices(torch.as_tensor(X), torch.as_tensor(lam), sf, sn)[2]
    resid = y - X @ n - c
    mean, var, mu_g, var_g = nominal_step(Ky_inv, torch.as_tensor(lam), torch.as_tensor(u), torch.as_tensor(s), torch.as_tensor(X),
                                          torch.as_tensor(resid), sf, n, c)
    qm, qv = quadrature_moments(X, resid, Ky_inv.numpy(), lam, sf, u, s, n, c)
    print("case %d: mean %.15g vs quadrature %.15g, var %.15g vs %.15g" % (case, mean.item(), qm, var.item(), qv))
    assert abs(mean.item() - qm) <= 1e-9 * max(1.0, abs(qm))
    assert abs(var.item() - qv) <= 1e-9
    if case < 2:                                                                  # the linear part moves both moments
        assert abs(mean.item() - mu_g.item()) > 1e-3 and abs(var.item() - var_g.item()) > 1e-6
