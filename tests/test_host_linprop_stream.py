"""What the choice between the two forms of the linearised step (include/gpmpc.h, "Linearised propagation": TILE, STREAM, AUTO) promises
without a device (CPU): the setter and its constants in the library, _lib.py and the header; the workspace queries under each form; the
Python surface (``linearised_form``, ``form=``, ``RiskSensitiveMPC.linearised_form``).  Every test leaves the process-wide form as it
found it."""
import ctypes
import os
import re

import pytest

import test_host_linprop as HT

ROOT = HT.ROOT
E_ARG = HT.E_ARG
CONSTANTS = ["LINPROP_FORM_TILE", "LINPROP_FORM_STREAM", "LINPROP_FORM_AUTO", "LINPROP_FORM_DEFAULT", "LINPROP_STREAM_COLS", "LINPROP_AUTO_MAX_B"]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_mpc_amd import _lib
    return _lib.lib()


@pytest.fixture()
def restored(L):
    """The form at the start of a test is the form at its end."""
    old = L.gpmpc_linearised_set_form(-1)
    yield old
    L.gpmpc_linearised_set_form(old)
    assert L.gpmpc_linearised_set_form(-1) == old


def header_constants():
    hdr = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    out = {}
    for name in CONSTANTS:
        m = re.search(r"^#define GPMPC_%s\s+(\w+)" % name, hdr, flags=re.M)
        assert m, name
        out[name] = m.group(1)
    for name in CONSTANTS:                               # (GPMPC_LINPROP_FORM_DEFAULT is written as the name of a form)
        v = out[name]
        out[name] = int(out[v[len("GPMPC_"):]] if v.startswith("GPMPC_") else v)
    return out


def test_setter_and_constants_in_library_binding_and_header(L, restored):
    from gaussian_process_mpc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    assert re.search(r"\bint\s+gpmpc_linearised_set_form\s*\(\s*int\s+form\s*\)\s*;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert _lib.SIGNATURES["gpmpc_linearised_set_form"] == (ctypes.c_int, [ctypes.c_int])
    assert L.gpmpc_linearised_set_form is not None
    H = header_constants()
    for name in CONSTANTS:
        assert getattr(_lib, name) == H[name], name
    assert (H["LINPROP_FORM_TILE"], H["LINPROP_FORM_STREAM"], H["LINPROP_FORM_AUTO"]) == (0, 1, 2)
    assert H["LINPROP_FORM_DEFAULT"] == H["LINPROP_FORM_TILE"]
    assert H["LINPROP_STREAM_COLS"] in (4, 8) and H["LINPROP_AUTO_MAX_B"] >= 0
    for text in ("STREAM", "GPMPC_LINPROP_AUTO_MAX_B", "NOT bit for bit"):
        assert text in hdr, text


def test_set_query_refuse(L, restored):
    from gaussian_process_mpc_amd import _lib
    TILE, STREAM, AUTO = _lib.LINPROP_FORM_TILE, _lib.LINPROP_FORM_STREAM, _lib.LINPROP_FORM_AUTO
    assert restored == _lib.LINPROP_FORM_DEFAULT == TILE     # nothing before this test left another form behind
    assert L.gpmpc_linearised_set_form(-1) == TILE
    assert L.gpmpc_linearised_set_form(STREAM) == TILE and L.gpmpc_linearised_set_form(-1) == STREAM
    assert L.gpmpc_linearised_set_form(AUTO) == STREAM and L.gpmpc_linearised_set_form(-1) == AUTO
    for bad in (3, -2):
        assert L.gpmpc_linearised_set_form(bad) == E_ARG
        assert "gpmpc_linearised_set_form" in L.gpmpc_last_error().decode()
        assert L.gpmpc_linearised_set_form(-1) == AUTO       # a refused call changes nothing
    assert L.gpmpc_linearised_set_form(TILE) == AUTO and L.gpmpc_linearised_set_form(-1) == TILE


QUERIES = [(4, 0, 0), (4, 1, 0), (1, 1, 0), (1, 0, 64), (65, 1, 64), (300, 1, 0), (5000, 0, 0)]
ROLL_QUERIES = [(4, 3, 0, 0), (4, 3, 1, 0), (1, 20, 1, 0), (1, 20, 0, 64), (300, 5, 1, 128)]


def test_workspace_queries_follow_the_form(L, restored):
    from gaussian_process_mpc_amd import _lib
    TILE, STREAM, AUTO = _lib.LINPROP_FORM_TILE, _lib.LINPROP_FORM_STREAM, _lib.LINPROP_FORM_AUTO
    models = [HT._model_c(), HT._model_c(n=300, ds=4, da=1), HT._model_c(n=2048, ds=4, da=1)]
    models[2].gp_stride = 2048 * 2048

    def ask():
        out = []
        for m in models:
            out += [L.gpmpc_linearised_step_workspace_bytes(ctypes.byref(m), *q) for q in QUERIES]
            out += [L.gpmpc_linearised_rollout_workspace_bytes(ctypes.byref(m), *q) for q in ROLL_QUERIES]
        return out

    def bad():
        g = models[0]
        return [L.gpmpc_linearised_step_workspace_bytes(ctypes.byref(g), 0, 1, 0), L.gpmpc_linearised_step_workspace_bytes(ctypes.byref(g), 4, 1, 100),
                L.gpmpc_linearised_rollout_workspace_bytes(ctypes.byref(g), 4, 3, 4, 0), L.gpmpc_linearised_rollout_workspace_bytes(ctypes.byref(g), 4, 0, 0, 0)]

    tile0 = ask()
    assert all(v > 0 for v in tile0) and bad() == [0, 0, 0, 0]
    # the TILE layout written out: Ks [np][C] | kpart [nbi][ds][1 + D][C] | part [ds][nbi][nv][C]  (| hpart | g), each rounded up to 256 bytes
    r256 = lambda b: (b + 255) // 256 * 256              # noqa: E731
    assert tile0[0] == r256(8 * 64 * 64) + r256(8 * 1 * 2 * 4 * 64) + r256(8 * 2 * 1 * 1 * 64)
    L.gpmpc_linearised_set_form(STREAM)
    stream = ask()
    assert all(v > 0 for v in stream) and bad() == [0, 0, 0, 0]
    L.gpmpc_linearised_set_form(AUTO)
    assert ask() == [max(a, b) for a, b in zip(tile0, stream)] and bad() == [0, 0, 0, 0]
    L.gpmpc_linearised_set_form(TILE)
    assert ask() == tile0                                # touching the setter changed nothing under TILE
    # the Jacobian costs workspace under STREAM too, and a workspace below the need is GPMPC_E_WORKSPACE under STREAM as under TILE
    L.gpmpc_linearised_set_form(STREAM)
    g = models[0]
    assert L.gpmpc_linearised_step_workspace_bytes(ctypes.byref(g), 4, 1, 0) > L.gpmpc_linearised_step_workspace_bytes(ctypes.byref(g), 4, 0, 0)
    p = ctypes.c_void_p
    a, b, c_, d, e = (p(0x2000 + 0x100 * i) for i in range(5))
    assert L.gpmpc_linearised_step(ctypes.byref(g), 4, a, b, c_, 1, d, e, None, 0, 0, p(0x9000), 16, None) == HT.E_WORKSPACE
    assert L.gpmpc_linearised_step(ctypes.byref(g), 4, a, b, c_, 1, d, e, None, 0, 100, p(0x9000), 1 << 40, None) == E_ARG    # chunk is still checked


def test_every_refusal_holds_under_stream(L, restored):
    from gaussian_process_mpc_amd import _lib
    L.gpmpc_linearised_set_form(_lib.LINPROP_FORM_STREAM)
    assert HT.check_refusals(L) >= 75


def test_python_surface(L, restored):
    import gaussian_process_mpc_amd as g
    from gaussian_process_mpc_amd import _lib, linearised
    assert g.linearised_form is linearised.linearised_form and "linearised_form" in g.__all__
    with pytest.raises(ValueError, match="form"):
        with g.linearised_form("bogus"):
            pass
    assert L.gpmpc_linearised_set_form(-1) == restored
    with g.linearised_form("stream"):
        assert L.gpmpc_linearised_set_form(-1) == _lib.LINPROP_FORM_STREAM
        with g.linearised_form("auto"):
            assert L.gpmpc_linearised_set_form(-1) == _lib.LINPROP_FORM_AUTO
        with g.linearised_form(None):
            assert L.gpmpc_linearised_set_form(-1) == _lib.LINPROP_FORM_STREAM
        assert L.gpmpc_linearised_set_form(-1) == _lib.LINPROP_FORM_STREAM
    assert L.gpmpc_linearised_set_form(-1) == restored
    with pytest.raises(RuntimeError, match="inside"):
        with g.linearised_form("stream"):
            raise RuntimeError("inside")
    assert L.gpmpc_linearised_set_form(-1) == restored     # restored on an exception
    # form="bogus" is a ValueError before the model is looked at, let alone anything launched
    for call in (lambda: g.linearised_step(None, None, None, None, form="bogus"), lambda: g.linearised_rollout(None, None, None, form="bogus"),
                 lambda: g.mppi_solve_linearised(None, None, None, None, form="bogus")):
        with pytest.raises(ValueError, match="form"):
            call()
    assert g.RiskSensitiveMPC.linearised_form is None
