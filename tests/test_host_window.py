"""CPU-only tests of the fixed-size training window's C ABI (gpmpc_kinv_remove, gpmpc_gp_replace): the symbols are exported and
declared, and every argument check answers before any device call, so it can be exercised without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpmpc_kinv_remove", "gpmpc_gp_replace_workspace_bytes", "gpmpc_gp_replace", "gpmpc_pack_callback_captures")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import gaussian_process_mpc_amd as g
    return g


def test_window_symbols_are_exported_and_declared(built):
    from gaussian_process_mpc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpmpc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gpmpc_[a-z_]+)\s*\(", hdr))
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(h, name) is not None
        assert getattr(built.lib(), name).argtypes == _lib.SIGNATURES[name][1]


def test_window_argument_validation_without_device(built):
    lib = built.lib()
    # host memory stands in for device buffers: every call below must be refused BEFORE anything is launched on them
    buf = [np.zeros(64) for _ in range(8)]
    a, b, c, d, e, f, x, ws = (ctypes.c_void_p(t.ctypes.data) for t in buf)
    lam = (ctypes.c_double * 3)(1.0, 1.0, 1.0)

    def remove(n=4, kin=a, ld_in=4, index=1, out=b, ld_out=3):
        return lib.gpmpc_kinv_remove(n, kin, ld_in, index, out, ld_out, None)

    assert remove(kin=None) == -1 and remove(out=None) == -1            # null pointers
    assert remove(n=1, index=0, ld_out=1) == -1 and remove(n=0, index=0) == -1      # n < 2
    assert remove(index=-1) == -1 and remove(index=4) == -1             # index out of range
    assert remove(out=a) == -1                                          # aliasing in / out
    assert remove(ld_in=3) == -1 and remove(ld_out=2) == -1             # leading dimensions too small

    nb = lib.gpmpc_gp_replace_workspace_bytes(4, 3)
    assert nb >= 3 * 4 * 8

    def replace(n=4, D=3, slot=1, X=x, xn=x, lp=lam, Kf=a, Ky=b, ldk=4, Ki=c, ld_in=4, Kfo=d, Kyo=e, Kio=f, ld_out=4, w=ws, wb=None):
        return lib.gpmpc_gp_replace(n, D, slot, X, xn, lp, 1.2, 1e-2, Kf, Ky, ldk, Ki, ld_in, Kfo, Kyo, Kio, ld_out, w,
                                    nb if wb is None else wb, None)

    for name in ("X", "xn", "lp", "Kf", "Ky", "Ki", "Kfo", "Kyo", "Kio", "w"):
        assert replace(**{name: None}) == -1, name                       # null pointers
    assert replace(n=0, slot=0) == -1
    assert replace(slot=-1) == -1 and replace(slot=4) == -1              # slot out of range
    assert replace(D=0) == -1 and replace(D=9) == -1                     # D > GPMPC_MAX_D
    assert replace(Kfo=a) == -1 and replace(Kyo=b) == -1 and replace(Kio=c) == -1    # aliasing in / out
    assert replace(ldk=3) == -1 and replace(ld_in=3) == -1 and replace(ld_out=3) == -1
    assert replace(wb=nb - 8) == -4 and replace(wb=0) == -4              # GPMPC_E_WORKSPACE


def test_replace_workspace_size_is_monotone(built):
    lib = built.lib()
    assert lib.gpmpc_pack_callback_captures(None) == 0
    assert lib.gpmpc_gp_replace_workspace_bytes(0, 3) == 0
    sizes = [lib.gpmpc_gp_replace_workspace_bytes(n, 3) for n in (1, 2, 63, 64, 65, 256, 1000, 4096)]
    assert all(s2 > s1 for s1, s2 in zip(sizes, sizes[1:])), sizes
    for n, s in zip((1, 2, 63, 64, 65, 256, 1000, 4096), sizes):
        assert s >= 3 * n * 8                                            # v, w and the kernel vector
